"""Running the detector over DATASETS.TEST and scoring what it finds: the functions behind ``tools/infer_net.py``
(``run_datasets``, ``save_evaluation``, ``save_visualizations``, ``run_rpn_recall``) and the evaluation a TRAINING process
runs on itself (``evaluate_in_training``: maskrcnn_benchmark/engine/trainer.py:174-203, the SOLVER.TEST_PERIOD block).

The two differ in what they keep.  ``run_datasets`` is the tool's route: the detections of every rank are gathered on rank 0,
saved as ``predictions.pth`` and scored there (engine/coco_eval.py::evaluate_coco).  ``evaluate_in_training`` keeps nothing
but the numbers -- the reference passes ``output_folder=None`` here -- so nothing is gathered: every rank scores the images it
predicted on its own device and only the match tables travel (engine/coco_eval.py::evaluate_coco_sharded).

``evaluate_in_training`` runs between two iterations of a live training process and leaves it as it found it: the mode flag
of every module, the class-embedding matrix (the very tensor it is handed back), torch's host and device random generators
(a ``DataLoader`` iterator draws its base seed from the host one).  It reads the weights through the model's own evaluation
pass, so it sees what the last optimizer step wrote: operands of trainable weights are never cached (layers/derived.py) and
the operands prepared ahead were prepared BEHIND that step (layers/pair_bottleneck.py::WeightPrepPlan).  It does not call the
training forward, so ``model.iter`` and the samplers' call counters do not move, and it builds an input transform of its own,
so the training transform's seeded draws do not move either.
"""
import json
import logging
import os
import time
from collections import OrderedDict

import torch

from . import coco_eval, coco_results, comm, error_analysis, inference, proposal_recall, visualize
from ..data.build import build_dataset, make_data_loader
from ..data.prefetch import DevicePrefetcher
from ..data.transforms import build_transforms


def save_visualizations(dataset, predictions, folder, count, threshold, device):
    """The first ``count`` images of ``dataset`` with their detections drawn (engine/visualize.py) -> ``folder``/<stem>.png."""
    from PIL import Image

    os.makedirs(folder, exist_ok=True)
    unseen = [dataset.json_category_id_to_contiguous_id[c] for c in dataset.class_splits.get("unseen", [])]
    for idx in range(min(count, len(predictions), len(dataset))):
        image = dataset.original_image(idx)  # RGB, at its own size, before any transform
        picture = visualize.render_predictions(image, predictions[idx].to(device), dataset.class_names, threshold=threshold,
                                               unseen_labels=unseen)
        stem = os.path.splitext(os.path.basename(dataset.get_img_info(idx)["file_name"]))[0]
        Image.fromarray(picture).save(os.path.join(folder, stem + ".png"))


def results_file_name(lvis=False, iteration=None):
    """``coco_results.json`` / ``coco_results_<iteration:07d>.json``; under LVIS-style federated rules ``lvis_results*`` -- the
    two sets of numbers cannot be mistaken for each other."""
    stem = "lvis_results" if lvis else "coco_results"
    return stem + ".json" if iteration is None else "{}_{:07d}.json".format(stem, iteration)


def save_evaluation(dataset, predictions, folder, iou_types, device, logger, recall=False, lvis=False, errors=False):
    """COCO scoring of one test set (engine/coco_eval.py): the table goes to the log, the numbers to
    ``folder``/coco_results.json as {iou_type: {metric: value}}.  ``recall``: the reference's whole table -- a
    ``box_proposal`` task first (engine/proposal_recall.py: the detections scored as proposals by their ``scores``, which is
    what the reference's table shows, its post-processor copying ``scores`` into ``objectness``), and the AR keys behind the
    AP keys of every iou_type.  ``lvis``: every iou_type under LVIS-style federated rules (``evaluate_coco(rules="lvis")``:
    APr / APc / APf, AR@300; the annotation file must be federatedly annotated), written to ``lvis_results.json``; the
    ``box_proposal`` task keeps its own rules.  ``errors``: the error analysis of engine/error_analysis.py for bbox and segm
    from the SAME scoring pass -- an ``errors_bbox`` / ``errors_segm`` table behind the others in the log and
    ``folder``/error_analysis.json; ``coco_results.json`` is byte for byte what it is without it."""
    if errors and lvis:
        raise ValueError("save_evaluation: the error analysis follows COCO's rules only; it does not go with lvis=True")
    rules = {"rules": "lvis"} if lvis else {}
    scored = {}
    if errors:
        rules = {"error_thresholds": (error_analysis.FG_THRESHOLD, error_analysis.BG_THRESHOLD), "tables_out": scored}
    if recall:
        results = OrderedDict(box_proposal=proposal_recall.evaluate_box_proposals(dataset, predictions, device, "scores"))
        results.update(coco_eval.evaluate_coco(dataset, predictions, iou_types, device, recall=True, **rules))
    else:
        results = coco_eval.evaluate_coco(dataset, predictions, iou_types, device, **rules)
    logger.info(coco_eval.format_results(results))
    with open(os.path.join(folder, results_file_name(lvis)), "w") as f:
        json.dump(results, f, indent=1)
    if errors:
        analysis = error_analysis.analyze_scored(dataset, scored, scored["cat_ids"])
        logger.info(coco_eval.format_results(error_analysis.task_tables(analysis)))
        with open(os.path.join(folder, "error_analysis.json"), "w") as f:
            json.dump(analysis, f, indent=1)
    return results


def run_rpn_recall(cfg, model, catalog, device, logger=None, folder="inference"):
    """(``folder``: ``inference_ema`` when the model holds the averaged weights, see ``run_datasets``.)Backbone + RPN alone over every DATASETS.TEST name (``model.propose``): the MODEL.RPN.POST_NMS_TOP_N_TEST proposals
    of every image, gathered like detections and saved as ``<OUTPUT_DIR>/inference/<name>/proposals.pth``, and on rank 0
    their box-proposal recall by ``objectness`` (engine/proposal_recall.py) as a ``rpn_proposal`` task in the log and in
    ``rpn_recall.json`` -> {name: the numbers (rank 0) or None}."""
    if not cfg.OUTPUT_DIR:
        raise ValueError("run_rpn_recall writes OUTPUT_DIR/inference/<name>/proposals.pth and rpn_recall.json: set OUTPUT_DIR")
    logger = logger or logging.getLogger("ovis.inference")
    transform = build_transforms(cfg, is_train=False)
    results = {}
    for name in cfg.DATASETS.TEST:
        dataset = build_dataset(cfg, name, catalog)
        loader = make_data_loader(cfg, dataset, transform, False, comm.get_rank(), comm.get_world_size())
        batches = DevicePrefetcher(loader, device, depth=2, transform=transform)
        out = os.path.join(cfg.OUTPUT_DIR, folder, name)
        try:
            proposals = inference.inference(model, batches, name, device, out, logger=logger, forward=model.propose,
                                            file_name="proposals.pth")
        finally:
            batches.close()
        results[name] = None
        if proposals is not None:
            results[name] = OrderedDict(rpn_proposal=proposal_recall.evaluate_box_proposals(dataset, proposals, device,
                                                                                            "objectness"))
            logger.info(coco_eval.format_results(results[name]))
            with open(os.path.join(out, "rpn_recall.json"), "w") as f:
                json.dump(results[name], f, indent=1)
    return results


def scored_iou_types(cfg, boundary_ap=False):
    """The tasks of a scoring run: bbox, segm when MODEL.MASK_ON, and -- ``boundary_ap`` -- boundary behind segm (Boundary AP
    is a mask metric: without MODEL.MASK_ON it is a ValueError)."""
    if boundary_ap and not cfg.MODEL.MASK_ON:
        raise ValueError("Boundary AP scores the mask head's masks: set MODEL.MASK_ON True")
    return ("bbox",) + (("segm",) if cfg.MODEL.MASK_ON else ()) + (("boundary",) if boundary_ap else ())


def run_datasets(cfg, model, catalog, device, logger=None, visualize_count=0, vis_threshold=0.5, evaluate=False,
                 export_results=False, recall=False, vote_thresh=None, average_masks=False, boundary_ap=False, lvis=False,
                 error_analysis=False, folder="inference"):
    """The detections of every DATASETS.TEST name -> {name: list of BoxLists (rank 0) or None}.  ``folder``: everything is
    written under OUTPUT_DIR/<folder>/<name>/ -- ``inference`` always means the raw weights, ``inference_ema`` the averaged
    ones (engine/ema.py; the caller has put them into the model).  ``vote_thresh`` /
    ``average_masks``: box voting and view-averaged masks of multi-scale / flip testing (engine/bbox_aug.py);
    ``boundary_ap``: with ``evaluate``, a ``boundary`` task behind ``segm`` (engine/coco_eval.py: Boundary AP); ``lvis``: with
    ``evaluate``, LVIS-style federated rules and ``lvis_results.json`` (``save_evaluation``); ``error_analysis``: with
    ``evaluate`` and without ``lvis``, the error tables and ``error_analysis.json`` (``save_evaluation(errors=True)``)."""
    if lvis and not evaluate:
        raise ValueError("run_datasets: lvis=True changes the rules of what evaluate=True scores")
    if error_analysis and (lvis or not evaluate):
        raise ValueError("run_datasets: error_analysis=True analyses what evaluate=True scores under COCO's rules")
    iou_types = scored_iou_types(cfg, boundary_ap and evaluate)
    transform = build_transforms(cfg, is_train=False)
    results = {}
    for name in cfg.DATASETS.TEST:
        dataset = build_dataset(cfg, name, catalog)
        loader = make_data_loader(cfg, dataset, transform, False, comm.get_rank(), comm.get_world_size())
        batches = DevicePrefetcher(loader, device, depth=2, transform=transform)
        out = os.path.join(cfg.OUTPUT_DIR, folder, name) if cfg.OUTPUT_DIR else None
        try:  # the zero-shot heads classify against THIS dataset's class embeddings
            results[name] = inference.inference(model, batches, name, device, out,
                                                class_embeddings=getattr(dataset, "class_emb_mtx", None), logger=logger,
                                                vote_thresh=vote_thresh, average_masks=average_masks)
        finally:
            batches.close()
        if visualize_count > 0 and out and results[name] is not None:  # rank 0 only: the others got None
            save_visualizations(dataset, results[name], os.path.join(out, "vis"), visualize_count, vis_threshold, device)
        if evaluate and not out:
            raise ValueError("run_datasets: evaluate=True writes OUTPUT_DIR/inference/<name>/coco_results.json: set OUTPUT_DIR")
        if export_results and not out:
            raise ValueError("run_datasets: export_results=True writes OUTPUT_DIR/inference/<name>/bbox.json and segm.json: "
                             "set OUTPUT_DIR")
        if evaluate and results[name] is not None:
            save_evaluation(dataset, results[name], out, iou_types, device, logger or logging.getLogger("ovis.inference"),
                            recall, lvis, *((True,) if error_analysis else ()))
        if export_results and results[name] is not None:
            coco_results.export_coco_results(dataset, results[name], out, ("bbox", "segm") if cfg.MODEL.MASK_ON else ("bbox",),
                                             device)
    return results


def evaluate_in_training(cfg, model, catalog, device, iteration, train_class_embeddings, logger=None, boundary_ap=False,
                         lvis=False, folder="inference"):
    """(``folder``: the results go under OUTPUT_DIR/<folder>/<name>/ -- ``inference_ema`` when the caller has put the averaged
    weights into the model, engine/ema.py::ModelEma.applied.)  The SOLVER.TEST_PERIOD evaluation of a live training process, behind iteration ``iteration`` (trainer.py:174-203):
    every DATASETS.TEST name through the model's evaluation pass on this rank's shard, scored where it was predicted
    (``coco_eval.evaluate_coco_sharded``: AP keys of ``bbox``, of ``segm`` when MODEL.MASK_ON, and of ``boundary`` behind it
    when ``boundary_ap``) -> {name: the numbers (rank 0) or None}.  Rank 0 logs the table under the iteration and writes
    ``OUTPUT_DIR/inference/<name>/coco_results_<iteration:07d>.json`` in the structure of ``coco_results.json``; no
    predictions are gathered or saved.  ``lvis``: LVIS-style federated rules (``evaluate_coco_sharded(rules="lvis")``), written
    to ``lvis_results_<iteration:07d>.json`` instead.  The caller has joined whatever else runs the model (``PipelinedTrainer.drain``).
    On return the model is as it was: every module's mode, ``train_class_embeddings`` as its class matrix (trainer.py:198-202),
    torch's random generators; a loader's worker processes live for one test set only."""
    if not cfg.OUTPUT_DIR:
        raise ValueError("evaluate_in_training writes OUTPUT_DIR/inference/<name>/coco_results_<iteration>.json: set OUTPUT_DIR")
    if cfg.TEST.BBOX_AUG.ENABLED:
        raise ValueError("evaluate_in_training scores one view per image: set TEST.BBOX_AUG.ENABLED False (tools/infer_net.py "
                         "runs multi-scale / flip testing on a checkpoint)")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("evaluate_in_training scores on the HIP device (mask IoU and matching have no host implementation)")
    logger = logger or logging.getLogger("ovis.trainer")
    iou_types = scored_iou_types(cfg, boundary_ap)
    comm.synchronize()
    modes = [(m, m.training) for m in model.modules()]
    host_rng, device_rng = torch.get_rng_state(), torch.cuda.get_rng_state(device)
    results = {}
    try:
        transform = build_transforms(cfg, is_train=False)
        for name in cfg.DATASETS.TEST:
            dataset = build_dataset(cfg, name, catalog)
            loader = make_data_loader(cfg, dataset, transform, False, comm.get_rank(), comm.get_world_size())
            batches = DevicePrefetcher(loader, device, depth=2, transform=transform)
            start = time.perf_counter()
            try:  # the zero-shot heads classify against THIS dataset's class embeddings; one without keeps the training set's
                embeddings = getattr(dataset, "class_emb_mtx", None)
                model.set_class_embeddings(train_class_embeddings if embeddings is None else embeddings.to(device))
                predictions = inference.compute_on_dataset(model, batches, device)
            finally:
                batches.close()
            comm.synchronize()
            predicted = time.perf_counter()
            results[name] = coco_eval.evaluate_coco_sharded(dataset, predictions, iou_types, device,
                                                            **({"rules": "lvis"} if lvis else {}))
            scored = time.perf_counter()
            logger.info("iteration %d, %s: %d images on this rank, inference %.2f s, scoring %.2f s", iteration, name,
                        len(predictions), predicted - start, scored - predicted)
            if results[name] is not None:
                logger.info("iteration %d, %s:%s", iteration, name, coco_eval.format_results(results[name]))
                out = os.path.join(cfg.OUTPUT_DIR, folder, name)
                os.makedirs(out, exist_ok=True)
                with open(os.path.join(out, results_file_name(lvis, iteration)), "w") as f:
                    json.dump(results[name], f, indent=1)
    finally:
        model.train()
        for module, mode in modes:  # the frozen RPN and the teacher heads were in eval mode inside the training step
            module.training = mode
        model.set_class_embeddings(train_class_embeddings)
        torch.set_rng_state(host_rng)
        torch.cuda.set_rng_state(device_rng, device)
    comm.synchronize()
    return results
