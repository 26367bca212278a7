"""Inference over the user's COCO-format files, with the command line of ``tools/test_net.py`` plus the catalog:

    python -m torch.distributed.run --nproc-per-node N tools/infer_net.py --config-file CFG --dataset-catalog FILE
        [--data-dir DIR] [--ckpt FILE] [--ema] KEY VALUE ...

One process per GPU; the weights come from ``--ckpt`` / ``MODEL.WEIGHT`` / the last checkpoint of OUTPUT_DIR
(utils/checkpoint.py).  Every name of DATASETS.TEST is resolved through the catalog (data/catalog.py), read through the raw
input path (data/build.py: loader workers decode and pack, the device makes the pixels), classified against the class
embeddings of its own annotation file (maskrcnn_benchmark/engine/inference.py:124-131), gathered on rank 0 and saved as
``<OUTPUT_DIR>/inference/<name>/predictions.pth``: a list of BoxLists in dataset-index order, at the transformed image
sizes.  ``--visualize N`` (rank 0) also renders the first N images of every test set -- boxes, filled masks, class names
(engine/visualize.py; detections scoring above ``--vis-threshold``) on the dataset's own decoded image -- to
``<OUTPUT_DIR>/inference/<name>/vis/<file stem>.png``.  ``--evaluate`` (rank 0, after the gather) scores every test set
against its own annotation file on the device (engine/coco_eval.py: COCO box AP, and mask AP when MODEL.MASK_ON, plus AP50
per class and per seen / unseen split), logs the reference's ``Task: ... / names / values`` table and writes
``<OUTPUT_DIR>/inference/<name>/coco_results.json``; it needs OUTPUT_DIR and MODEL.DEVICE cuda -- there is no host-only
scoring.  ``--recall`` (with ``--evaluate``) completes the reference's table: a ``box_proposal`` task first -- AR@100, ARs@100,
... ARl@1000 of the detections scored as class-agnostic proposals, and AR@<limit>_split_<split> (engine/proposal_recall.py, matched
on the device) -- and COCO's AR1 / AR10 / AR100 / ARs / ARm / ARl plus AR100_split_<split> behind the AP keys.
``--boundary-ap`` (with ``--evaluate`` and MODEL.MASK_ON) adds a ``boundary`` task behind ``segm``: Boundary AP (Cheng et al.,
CVPR 2021; engine/coco_eval.py), segm's keys from a matching on min(mask IoU, boundary IoU).  ``--lvis`` (with
``--evaluate``) scores every task under LVIS-style federated rules instead -- the annotation file carries
``neg_category_ids``, ``not_exhaustive_category_ids`` and ``frequency``; AP ... APl, APr, APc, APf, 300 detections per image
(engine/coco_eval.py ``rules="lvis"``; the rules are restated in include/ovis_hip.h and have not been compared with
lvis-api's output) -- and writes ``lvis_results.json`` in place of ``coco_results.json``; it combines with ``--boundary-ap``
and ``--recall``, whose ``box_proposal`` task keeps its own rules.  ``--error-analysis`` (with ``--evaluate``, not with ``--lvis``)
says WHY an AP50 is low: every false positive of the matching at IoU 0.5 is typed Cls, Loc, Both, Dupe or Bkg on the device
and every ground truth nobody found or aimed at is Miss (engine/error_analysis.py, csrc/error_types.hip; TIDE's decomposition
as include/ovis_hip.h restates it, not compared with tidecv's output); ``dAP50_<type>`` -- what AP50 would gain with that type
fixed, overall and per split -- goes to the log as ``errors_bbox`` / ``errors_segm`` tables and, with the error counts and the
split-by-split class confusion, to ``error_analysis.json``; ``coco_results.json`` is byte for byte what it is without the
flag, and a ``boundary`` task is scored as before and not analysed.  ``--rpn-recall``
is a run of its own: backbone + RPN alone (``model.propose``), the proposals gathered like detections into
``<OUTPUT_DIR>/inference/<name>/proposals.pth`` and scored by ``objectness`` as an ``rpn_proposal`` task, written to
``rpn_recall.json`` -- whether the RPN proposes the unseen classes at all.  ``--export-results`` (rank 0, after the gather, independent of ``--evaluate``) writes the detections as COCO results
files next to ``predictions.pth`` (engine/coco_results.py): ``bbox.json``, and ``segm.json`` when MODEL.MASK_ON -- every
detection, boxes as xywh and masks as compressed RLE at the ORIGINAL image sizes, the masks encoded on the device; it needs
OUTPUT_DIR, and MODEL.DEVICE cuda when MODEL.MASK_ON.  ``TEST.BBOX_AUG.ENABLED True`` (with H_FLIP / SCALES / MAX_SIZE / SCALE_H_FLIP) turns on multi-scale / flip testing:
``build_transforms(cfg, False)`` then makes every view on the device from the one upload and ``engine/bbox_aug.py`` merges the
views' detections; the saved BoxLists are in the first view's frame and keep their masks.  Two options of that mode, neither
in the reference: ``--bbox-vote THR`` replaces every kept box by the score-weighted mean of the merged candidates of its class
that overlap it by IoU >= THR (box voting), ``--mask-aug`` runs the mask head on every view and saves the mean of the views'
maps instead of the first view's (engine/bbox_aug.py).  ``--soft-nms {linear,gaussian}`` (with or without
TEST.BBOX_AUG.ENABLED; not in the reference either) replaces the greedy per-class NMS of the box post-processor by Soft-NMS
(Bodla et al., ICCV 2017; ``_C.soft_nms``, the rule in include/ovis_hip.h): overlapped candidates lose score instead of being
deleted, those that fall below ``--soft-nms-min-score`` (default MODEL.ROI_HEADS.SCORE_THRESH; Detectron: 0.0001) go, the saved
``scores`` are the decayed ones and DETECTIONS_PER_IMG ranks by them; ``--soft-nms-sigma`` (default 0.5) is the Gaussian's
width, the IoU threshold is MODEL.ROI_HEADS.NMS.  It composes with ``--bbox-vote`` (the vote weighs with the candidates'
original scores) and ``--mask-aug``.  ``tools/test_net.py`` stays the
synthetic-stream tool; LVIS scoring is outside this build.  ``--ema`` loads the checkpoint's ``"ema"`` entry (the weight
average of ``tools/train_net.py --ema``, engine/ema.py) over the model's trainable parameters before inference and writes
everything under ``<OUTPUT_DIR>/inference_ema/<name>/`` instead: ``inference_ema`` always means averaged weights, ``inference``
raw ones.  It only changes which weights are loaded, so it composes with every other flag; a checkpoint without the entry is
an error naming the file.
"""
import argparse
import json  # noqa: F401  (the module's names stay what they were before engine/evaluation.py took the functions)
import logging
import os
import sys
from collections import OrderedDict  # noqa: F401

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.build import build_dataset, make_data_loader  # noqa: E402,F401
from cvpr22_cross_modal_pseudo_labeling_amd.data.catalog import DatasetCatalog  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher  # noqa: E402,F401
from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import calibrate_stem_bn, make_batch, make_embeddings  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms  # noqa: E402,F401
from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import evaluating_post_processor  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval, coco_results, comm, inference, proposal_recall, visualize  # noqa: E402,F401
from cvpr22_cross_modal_pseudo_labeling_amd.engine.ema import load_ema_weights  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.engine.evaluation import (run_datasets, run_rpn_recall, save_evaluation,  # noqa: E402,F401
                                                                       save_visualizations)
from cvpr22_cross_modal_pseudo_labeling_amd.modeling.detector import build_detection_model  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import SoftNMS  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.utils.checkpoint import DetectronCheckpointer  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser(description="MI355X-native detection inference over COCO-format files")
    parser.add_argument("--config-file", default="", metavar="FILE", help="path to config file")
    parser.add_argument("--local_rank", type=int, default=int(os.environ.get("LOCAL_RANK", 0)))
    parser.add_argument("--ckpt", default=None, help="checkpoint to test instead of MODEL.WEIGHT / the last one of OUTPUT_DIR")
    parser.add_argument("--dataset-catalog", required=True, metavar="FILE",
                        help="JSON catalog {name: {img_dir, ann_file, ann_file_cap?, vocab_file?}} of the DATASETS.TEST names")
    parser.add_argument("--data-dir", default="", help="where the catalog's relative paths are taken from")
    parser.add_argument("--visualize", type=int, default=0, metavar="N",
                        help="render the first N images of every test set to OUTPUT_DIR/inference/<name>/vis/ (rank 0)")
    parser.add_argument("--vis-threshold", type=float, default=0.5, metavar="T", help="draw detections scoring above T")
    parser.add_argument("--evaluate", action="store_true",
                        help="score every test set on the device (COCO box / mask AP, AP50 per class and split) and write "
                             "OUTPUT_DIR/inference/<name>/coco_results.json (rank 0)")
    parser.add_argument("--export-results", action="store_true",
                        help="write every test set's detections as COCO results files, OUTPUT_DIR/inference/<name>/bbox.json "
                             "and (MODEL.MASK_ON) segm.json with the masks RLE-encoded on the device (rank 0)")
    parser.add_argument("--recall", action="store_true",
                        help="with --evaluate: the reference's whole table -- a box_proposal task first (AR@100 ... ARl@1000 of "
                             "the detections scored as proposals, and per split) and COCO AR1 / AR10 / AR100 / ARs / ARm / ARl "
                             "and AR100 per split behind the AP keys")
    parser.add_argument("--boundary-ap", action="store_true",
                        help="with --evaluate and MODEL.MASK_ON: also score Boundary AP (Cheng et al., CVPR 2021) -- a boundary "
                             "task behind segm in the table and in coco_results.json: segm's keys, matched on min(mask IoU, "
                             "boundary IoU)")
    parser.add_argument("--lvis", action="store_true",
                        help="with --evaluate: score under LVIS-style federated rules (neg_category_ids, "
                             "not_exhaustive_category_ids, frequency: AP ... APl, APr, APc, APf; 300 detections per image) and "
                             "write lvis_results.json in place of coco_results.json; box_proposal keeps its own rules")
    parser.add_argument("--error-analysis", action="store_true",
                        help="with --evaluate (not with --lvis): break AP50 down by error type from the same scoring pass -- "
                             "Cls, Loc, Both, Dupe, Bkg, Miss and the AP50 each would give back, per seen / unseen split -- as "
                             "errors_bbox / errors_segm tables in the log and OUTPUT_DIR/inference/<name>/error_analysis.json")
    parser.add_argument("--rpn-recall", action="store_true",
                        help="run backbone + RPN alone over every test set, save the proposals as "
                             "OUTPUT_DIR/inference/<name>/proposals.pth and score their recall by objectness on the device: an "
                             "rpn_proposal task in the log and in rpn_recall.json (rank 0); no detections are made")
    parser.add_argument("--bbox-vote", type=float, default=None, metavar="THR",
                        help="with TEST.BBOX_AUG.ENABLED True: box voting -- every kept box becomes the score-weighted mean of "
                             "the merged candidates of its class with IoU >= THR, a float in (0, 1]")
    parser.add_argument("--mask-aug", action="store_true",
                        help="with TEST.BBOX_AUG.ENABLED True and MODEL.MASK_ON: the masks are the mean of every view's "
                             "mask-head pass instead of the first view's")
    parser.add_argument("opts", default=None, nargs=argparse.REMAINDER, help="KEY VALUE overrides")
    # Soft-NMS's flags have a parser of their own, read first: the namespace of the parser above stays what it was
    soft_parser = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    soft_parser.add_argument("--soft-nms", choices=("linear", "gaussian"), default=None,
                             help="Soft-NMS (Bodla et al., ICCV 2017) in place of the greedy per-class NMS: overlapped "
                                  "candidates lose score (linear: x (1 - IoU) above MODEL.ROI_HEADS.NMS; gaussian: x exp(-IoU^2 "
                                  "/ sigma)) instead of being deleted; with or without TEST.BBOX_AUG.ENABLED")
    soft_parser.add_argument("--soft-nms-sigma", type=float, default=None, metavar="S",
                             help="with --soft-nms: the Gaussian's sigma, > 0 (default 0.5)")
    soft_parser.add_argument("--soft-nms-min-score", type=float, default=None, metavar="V",
                             help="with --soft-nms: a candidate whose decayed score falls below V >= 0 is dropped (default "
                                  "MODEL.ROI_HEADS.SCORE_THRESH; Detectron uses 0.0001)")
    parser.epilog = "Soft-NMS flags (in front of the KEY VALUE overrides, like every flag) -- " + "; ".join(
        f"{a.option_strings[0]} {a.metavar or '{' + ','.join(a.choices) + '}'}: {a.help}" for a in soft_parser._actions)
    soft, argv = soft_parser.parse_known_args(sys.argv[1:] if argv is None else argv)
    # ... and so has --ema (it only changes which weights are loaded and the folder everything is written under)
    ema_parser = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    ema_parser.add_argument("--ema", action="store_true",
                            help="test the checkpoint's \"ema\" entry (the weight average of tools/train_net.py --ema) instead "
                                 "of its raw weights, and write under OUTPUT_DIR/inference_ema/<name>/; a checkpoint without "
                                 "the entry is an error")
    parser.epilog += ".  --ema (in front of the overrides too): " + ema_parser._actions[0].help
    averaged, argv = ema_parser.parse_known_args(argv)
    args = parser.parse_args(argv)

    world = int(os.environ.get("WORLD_SIZE", 1))
    cfg = get_defaults()
    if args.config_file:
        cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(args.opts or [])
    cfg.freeze()
    if args.visualize > 0 and not cfg.OUTPUT_DIR:
        parser.error("--visualize writes under OUTPUT_DIR/inference/<name>/vis/: set OUTPUT_DIR")
    if args.evaluate and not cfg.OUTPUT_DIR:
        parser.error("--evaluate writes OUTPUT_DIR/inference/<name>/coco_results.json: set OUTPUT_DIR")
    if args.evaluate and cfg.MODEL.DEVICE != "cuda":
        parser.error("--evaluate scores on the HIP device (mask IoU and matching have no host implementation): "
                     "set MODEL.DEVICE cuda")
    if args.recall and not args.evaluate:
        parser.error("--recall adds the recall numbers to what --evaluate scores: give --evaluate too")
    if args.lvis and not args.evaluate:
        parser.error("--lvis changes the rules of what --evaluate scores: it is valid only with --evaluate")
    if args.error_analysis and not args.evaluate:
        parser.error("--error-analysis analyses what --evaluate scores: it is valid only with --evaluate")
    if args.error_analysis and args.lvis:
        parser.error("--error-analysis follows COCO's rules: it does not go with --lvis (under federated annotation an "
                     "unannotated object makes the background error meaningless)")
    if args.boundary_ap and not args.evaluate:
        parser.error("--boundary-ap adds the boundary task to what --evaluate scores: give --evaluate too")
    if args.boundary_ap and not cfg.MODEL.MASK_ON:
        parser.error("--boundary-ap scores the mask head's masks: set MODEL.MASK_ON True")
    if args.rpn_recall and not cfg.OUTPUT_DIR:
        parser.error("--rpn-recall writes OUTPUT_DIR/inference/<name>/proposals.pth and rpn_recall.json: set OUTPUT_DIR")
    if args.rpn_recall and cfg.MODEL.DEVICE != "cuda":
        parser.error("--rpn-recall matches proposals and ground truth on the HIP device (no host implementation): "
                     "set MODEL.DEVICE cuda")
    if args.rpn_recall and (args.evaluate or args.export_results or args.visualize > 0):
        parser.error("--rpn-recall makes no detections: it does not go with --evaluate, --export-results or --visualize")
    if args.rpn_recall and cfg.TEST.BBOX_AUG.ENABLED:
        parser.error("--rpn-recall scores the proposals of one view: set TEST.BBOX_AUG.ENABLED False")
    if args.export_results and not cfg.OUTPUT_DIR:
        parser.error("--export-results writes OUTPUT_DIR/inference/<name>/bbox.json and segm.json: set OUTPUT_DIR")
    if args.export_results and cfg.MODEL.MASK_ON and cfg.MODEL.DEVICE != "cuda":
        parser.error("--export-results encodes the masks of segm.json on the HIP device (the run-length encoder has no host "
                     "implementation): set MODEL.DEVICE cuda")
    if soft.soft_nms is None and (soft.soft_nms_sigma is not None or soft.soft_nms_min_score is not None):
        parser.error("--soft-nms-sigma / --soft-nms-min-score are parameters of Soft-NMS: they are valid only with --soft-nms")
    if soft.soft_nms_sigma is not None and not soft.soft_nms_sigma > 0.0:
        parser.error(f"--soft-nms-sigma takes a width > 0, got {soft.soft_nms_sigma}")
    if soft.soft_nms_min_score is not None and not soft.soft_nms_min_score >= 0.0:
        parser.error(f"--soft-nms-min-score takes a score >= 0, got {soft.soft_nms_min_score}")
    if soft.soft_nms is not None and args.rpn_recall:
        parser.error("--soft-nms acts on the detections' post-processing and --rpn-recall makes no detections: they do not go "
                     "together")
    if soft.soft_nms is not None and cfg.MODEL.DEVICE != "cuda":
        parser.error("--soft-nms is an option of the HIP device's post-processing: set MODEL.DEVICE cuda")
    if soft.soft_nms is not None and cfg.MODEL.GT_BOX_EVAL:
        parser.error("--soft-nms does not go with MODEL.GT_BOX_EVAL True: every ground-truth box is kept by definition")
    if args.bbox_vote is not None and not cfg.TEST.BBOX_AUG.ENABLED:
        parser.error("--bbox-vote votes over the views of multi-scale / flip testing: set TEST.BBOX_AUG.ENABLED True")
    if args.mask_aug and not cfg.TEST.BBOX_AUG.ENABLED:
        parser.error("--mask-aug averages the masks of the views of multi-scale / flip testing: set TEST.BBOX_AUG.ENABLED True")
    if args.mask_aug and not cfg.MODEL.MASK_ON:
        parser.error("--mask-aug averages the mask head's maps: set MODEL.MASK_ON True")
    if args.bbox_vote is not None and not 0.0 < args.bbox_vote <= 1.0:
        parser.error(f"--bbox-vote takes an IoU threshold in (0, 1], got {args.bbox_vote}")
    device = torch.device(cfg.MODEL.DEVICE, args.local_rank) if cfg.MODEL.DEVICE == "cuda" else torch.device(cfg.MODEL.DEVICE)
    if cfg.MODEL.DEVICE == "cuda":
        torch.cuda.set_device(args.local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl" if cfg.MODEL.DEVICE == "cuda" else "gloo", init_method="env://")
        comm.synchronize()
    logging.basicConfig(level=logging.INFO if comm.get_rank() == 0 else logging.WARNING,
                        format="%(asctime)s %(name)s %(levelname)s: %(message)s")
    logger = logging.getLogger("ovis.inference")
    logger.info("Using %d GPUs\n%s %s%s", world, args, soft, " --ema" if averaged.ema else "")

    catalog = DatasetCatalog(args.dataset_catalog, args.data_dir)
    model = build_detection_model(cfg).to(device)
    checkpointer = DetectronCheckpointer(cfg, model, save_dir=cfg.OUTPUT_DIR)
    weight = args.ckpt or cfg.MODEL.WEIGHT
    extra = checkpointer.load(weight, use_latest=args.ckpt is None)
    if averaged.ema:
        source = checkpointer.get_checkpoint_file() if args.ckpt is None and checkpointer.has_checkpoint() else weight
        if "ema" not in extra:
            parser.error(f"--ema: the checkpoint {source or '(none given)'} has no \"ema\" entry (train with "
                         "tools/train_net.py --ema DECAY)")
        load_ema_weights(model, extra["ema"])
        logger.info("--ema: the averaged weights of %s (update count %d) over %d trainable tensors", source,
                    int(extra["ema"]["num_updates"]), len(extra["ema"]["params"]))
    if not weight and not extra and not checkpointer.has_checkpoint():
        images, _ = make_batch(1, device=device, seed=7)
        calibrate_stem_bn(model, images)  # random init only: give the frozen BN usable statistics
    _, e_seen = make_embeddings(cfg.MODEL.ROI_BOX_HEAD.EMB_DIM, device=device)
    model.set_class_embeddings(e_seen)  # stands until a dataset brings its own (DATASETS.DATASET_ARGS.LOAD_EMBEDDINGS)
    if soft.soft_nms is not None:
        post = evaluating_post_processor(model)
        post.soft_nms = SoftNMS(soft.soft_nms, 0.5 if soft.soft_nms_sigma is None else soft.soft_nms_sigma,
                                post.score_thresh if soft.soft_nms_min_score is None else soft.soft_nms_min_score)
        logger.info("Soft-NMS in place of the per-class NMS: %s, Nt %s", post.soft_nms, post.nms)
    if args.rpn_recall:
        run_rpn_recall(cfg, model, catalog, device, logger, **({"folder": "inference_ema"} if averaged.ema else {}))
    else:
        for name, preds in run_datasets(cfg, model, catalog, device, logger, args.visualize, args.vis_threshold,
                                        args.evaluate, args.export_results, args.recall, args.bbox_vote,
                                        args.mask_aug, args.boundary_ap, args.lvis,
                                        **({"error_analysis": True} if args.error_analysis else {}),
                                        **({"folder": "inference_ema"} if averaged.ema else {})).items():
            if preds is not None:
                logger.info("%s: %d images, %d detections", name, len(preds), sum(len(p) for p in preds))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
