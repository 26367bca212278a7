"""Training entry point with the reference's command line (tools/train_net.py:162-234):

    python -m torch.distributed.run --nproc-per-node N tools/train_net.py --config-file CFG [--dataset-catalog FILE]
        [--color-jitter] [--scale-jitter LO HI [--crop-size H W] [--copy-paste P]] [--evaluate] [--boundary-ap] [--lvis] [--skip-test] [--ema DECAY] KEY VALUE ...

One process per GPU (RCCL via torch.distributed, env:// rendezvous), config = defaults <- yaml <- trailing overrides,
frozen before use.  Without ``--dataset-catalog`` the data stream is the synthetic COCO-shaped generator
(cvpr22_cross_modal_pseudo_labeling_amd/data/synthetic.py); with it, DATASETS.TRAIN is read from the user's COCO-format
files (data/catalog.py, data/datasets.py, data/build.py) through the raw input path.  MODEL.WEIGHT (a ``.pth`` in the reference's wire format),
OUTPUT_DIR resume and SOLVER.CHECKPOINT_PERIOD behave as in the reference (utils/checkpoint.py: checkpoints are written and
resumed from whenever OUTPUT_DIR is set; ``--no-checkpoints`` opts out).  ``--color-jitter`` (with ``--raw-input`` or
``--dataset-catalog``) makes the training transform honour INPUT.BRIGHTNESS / CONTRAST / SATURATION / HUE: the reference's
ColorJitter in front of the resize, drawn in the loader and run on the device (data/transforms.py); off by default.
``--copy-paste P`` (with ``--scale-jitter``, MODEL.MASK_ON and MODEL.DEVICE cuda; polygon ground truth) pastes, with
probability P per image, a random half of the neighbouring image's instances over it at the same canvas position: decided in
the loader, masks and pixels composited on the device (include/ovis_hip.h states the rule; off by default).

``--evaluate`` (with ``--dataset-catalog``, OUTPUT_DIR and MODEL.DEVICE cuda) is the reference's evaluation while training:
behind every SOLVER.TEST_PERIOD-th iteration -- counted over the whole run, after that iteration's checkpoint -- every
DATASETS.TEST set goes through the model as it stands and its COCO box AP (mask AP when MODEL.MASK_ON, AP50 per class and
per seen / unseen split) is logged under the iteration and written to
``OUTPUT_DIR/inference/<name>/coco_results_<iteration:07d>.json`` (engine/evaluation.py::evaluate_in_training,
maskrcnn_benchmark/engine/trainer.py:174-203: every rank scores the images it predicted, nothing is saved but the numbers);
and after the last iteration the final test (tools/train_net.py:129-159 of the reference), which is what
``tools/infer_net.py --evaluate`` does with the final weights -- ``predictions.pth`` and ``coco_results.json`` under
``OUTPUT_DIR/inference/<name>/`` -- unless ``--skip-test``.  ``--boundary-ap`` (with ``--evaluate`` and MODEL.MASK_ON) adds
Boundary AP to both: a ``boundary`` task behind ``segm`` in every table and ``coco_results*.json`` (engine/coco_eval.py).  ``--lvis`` (with ``--evaluate``) scores both
under LVIS-style federated rules -- APr / APc / APf of an annotation file with ``neg_category_ids``,
``not_exhaustive_category_ids`` and ``frequency`` (engine/coco_eval.py ``rules="lvis"``; the rules are restated in
include/ovis_hip.h and have not been compared with lvis-api's output) -- and writes ``lvis_results*.json`` in place of
``coco_results*.json``.  Without ``--evaluate`` neither runs and ``--skip-test`` has
nothing to skip.  The validation loss of the reference's loop is not computed (every shipped yaml sets
SOLVER.SKIP_VAL_LOSS True; the reference's version runs the training forward, which moves the student-teacher model's
iteration count), TEST.BBOX_AUG belongs to ``tools/infer_net.py``, and TensorBoard and best-checkpoint tracking are outside
this build.

``--ema DECAY`` (a float in (0, 1)) keeps an exponential moving average of every trainable parameter, moved inside the fused
SGD launch at every optimizer step (engine/ema.py, csrc/optim.hip; include/ovis_hip.h states the rule:
d_t = min(DECAY, (1 + t) / (10 + t)), fp32 averages, made behind the checkpoint load, one per rank and no collective).  Every
checkpoint carries it as its ``"ema"`` entry, and a resumed run restores it (MODEL.LOAD_TRAINER_STATE).  With ``--evaluate`` the
periodic scoring runs on the AVERAGED weights and writes ``OUTPUT_DIR/inference_ema/<name>/coco_results_<iteration:07d>.json``,
and the final test runs twice: on the raw weights into ``inference/`` as without the flag, then on the averaged ones into
``inference_ema/``.  ``inference_ema`` always means averaged weights, ``inference`` always raw.  Without the flag nothing
changes: no tensor, no launch, no checkpoint key, no file.
"""
import argparse
import functools
import logging
import os
import sys

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this driver: RCCL between ranks needs it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvpr22_cross_modal_pseudo_labeling_amd.engine import launch  # noqa: E402  (no torch, no GPU)

# pin this rank to its share of the cores (of its GPU's NUMA node when sysfs tells) before torch / HIP start their threads
AFFINITY = launch.apply_rank_affinity() if __name__ == "__main__" else {"cpus": None, "source": "not applied"}

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.build import build_train_dataset, make_data_loader  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.catalog import DatasetCatalog  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import (LVIS_VOCAB, RawSyntheticBatches,  # noqa: E402
                                                                       SyntheticBatches, calibrate_stem_bn, make_batch,
                                                                       make_embeddings)
from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import (JITTER_KEYS, build_transforms, check_color_jitter,  # noqa: E402
                                                                        check_copy_paste, check_scale_jitter)
from cvpr22_cross_modal_pseudo_labeling_amd.engine import comm, evaluation, solver, trainer  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.engine.ema import ModelEma  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.modeling.detector import build_detection_model  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.utils.checkpoint import DetectronCheckpointer  # noqa: E402


def make_data_source(cfg, ims_per_gpu, raw_input=False, dataset=None, start_iter=0, max_iter=None, seed=0, color_jitter=False,
                     scale_jitter=None, crop_size=None, copy_paste=None):
    """-> (loader of host batches, the input transform or None).  ``dataset`` (``--dataset-catalog``): the reference's
    batching over the user's files (data/build.py), counted from ``start_iter``, its size and flip draws seeded by ``seed``;
    otherwise the endless synthetic streams.  ``color_jitter``: the transform honours INPUT.BRIGHTNESS / CONTRAST /
    SATURATION / HUE (data/transforms.py).  ``scale_jitter`` = (lo, hi), ``crop_size`` = (height, width): large-scale jitter
    on a fixed canvas, behind the colour jitter when both are on.  ``copy_paste`` = P: copy-paste between the images of a
    batch on that canvas (it needs ``scale_jitter``)."""
    if color_jitter and not (raw_input or dataset is not None):
        raise ValueError("color_jitter acts on raw uint8 images: it needs raw_input or a dataset")
    if scale_jitter is not None and not (raw_input or dataset is not None):
        raise ValueError("scale_jitter acts in the device input transform: it needs raw_input or a dataset")
    if crop_size is not None and scale_jitter is None:
        raise ValueError("crop_size is the canvas of scale_jitter: give scale_jitter too")
    if copy_paste is not None and scale_jitter is None:
        raise ValueError("copy_paste pastes at the same position of a fixed canvas: give scale_jitter too")
    transform = (build_transforms(cfg, is_train=True, color_jitter=color_jitter, scale_jitter=scale_jitter, crop_size=crop_size,
                                  copy_paste=copy_paste)
                 if (raw_input or dataset is not None) else None)
    if dataset is not None:
        return make_data_loader(cfg, dataset, transform, True, comm.get_rank(), comm.get_world_size(), start_iter=start_iter,
                                seed=seed, max_iter=max_iter), transform
    source = (RawSyntheticBatches(ims_per_gpu, transform, seed0=1234, rank=comm.get_rank()) if raw_input
              else SyntheticBatches(ims_per_gpu, seed0=1234, rank=comm.get_rank()))
    loader = torch.utils.data.DataLoader(source, batch_size=None,
                                         num_workers=cfg.DATALOADER.NUM_WORKERS,
                                         prefetch_factor=2 if cfg.DATALOADER.NUM_WORKERS > 0 else None,
                                         persistent_workers=cfg.DATALOADER.NUM_WORKERS > 0)
    return loader, transform


def train(cfg, local_rank, distributed, max_iter, ims_per_gpu, save_checkpoints=False, raw_input=False, dataset_catalog=None,
          data_dir="", seed=0, evaluate=False, skip_test=False, boundary_ap=False, lvis=False, color_jitter=False,
          scale_jitter=None, crop_size=None, copy_paste=None, ema_decay=None):
    """``ema_decay`` = DECAY in (0, 1): a weight average moved by every optimizer step (engine/ema.py), saved with every
    checkpoint, scored by the periodic evaluation and by a second final test, both into OUTPUT_DIR/inference_ema/.
    ``evaluate``: score every DATASETS.TEST set behind every SOLVER.TEST_PERIOD-th iteration
    (engine/evaluation.py::evaluate_in_training) and, unless ``skip_test``, run the final test behind the last one
    (``evaluation.run_datasets``: predictions.pth and coco_results.json under OUTPUT_DIR/inference/<name>/).
    ``boundary_ap``: both also score the ``boundary`` task (engine/coco_eval.py: Boundary AP), behind ``segm``.  ``lvis``:
    both score under LVIS-style federated rules and write ``lvis_results*.json`` instead.  ``color_jitter``: the raw input
    path jitters the training images as INPUT.BRIGHTNESS / CONTRAST / SATURATION / HUE say.  ``scale_jitter`` / ``crop_size``:
    it trains on large-scale-jittered crops of a fixed canvas; the periodic and the final test use the plain test transform.
    ``copy_paste`` = P in (0, 1]: copy-paste between the images of a training batch (with ``scale_jitter``, MODEL.MASK_ON and
    MODEL.DEVICE cuda)."""
    if copy_paste is not None and (cfg.MODEL.DEVICE != "cuda" or not cfg.MODEL.MASK_ON):
        raise ValueError("train(copy_paste=P) composites masks on the HIP device: it needs MODEL.DEVICE cuda and MODEL.MASK_ON True")
    if lvis and not evaluate:
        raise ValueError("train(lvis=True) changes the rules of what evaluate=True scores")
    if boundary_ap and not evaluate:
        raise ValueError("train(boundary_ap=True) adds a task to what evaluate=True scores")
    if boundary_ap and not cfg.MODEL.MASK_ON:
        raise ValueError("train(boundary_ap=True) scores the mask head's masks: set MODEL.MASK_ON True")
    if evaluate and not (dataset_catalog and cfg.OUTPUT_DIR and cfg.MODEL.DEVICE == "cuda"):
        raise ValueError("train(evaluate=True) needs a dataset catalog (DATASETS.TEST), OUTPUT_DIR and MODEL.DEVICE cuda")
    if evaluate and cfg.TEST.BBOX_AUG.ENABLED:
        raise ValueError("train(evaluate=True) scores one view per image: set TEST.BBOX_AUG.ENABLED False")
    device = torch.device(cfg.MODEL.DEVICE, local_rank) if cfg.MODEL.DEVICE == "cuda" else torch.device(cfg.MODEL.DEVICE)
    model = build_detection_model(cfg).to(device)
    catalog = DatasetCatalog(dataset_catalog, data_dir) if dataset_catalog else None
    dataset = build_train_dataset(cfg, catalog) if catalog is not None else None
    # the caption-vocabulary matrix stays the seeded stand-in: as many rows as the dataset's vocabulary when that is larger
    n_vocab = max(LVIS_VOCAB, len(dataset.parser.class_names) if getattr(dataset, "parser", None) else 0)
    e_vocab, e_seen = make_embeddings(cfg.MODEL.ROI_BOX_HEAD.EMB_DIM, device=device, n_vocab=n_vocab)
    if dataset is not None and cfg.DATASETS.DATASET_ARGS.LOAD_EMBEDDINGS:
        e_seen = dataset.class_emb_mtx.to(device)  # the class embeddings of the annotation file (datasets/coco.py:74-91)
    model.set_class_embeddings(e_seen)  # engine/trainer.py:85-90
    if hasattr(model, "set_caption_vocab"):
        model.set_caption_vocab(e_vocab)
    optimizer = solver.make_optimizer(cfg, model)
    scheduler = solver.make_lr_scheduler(cfg, optimizer)
    # tools/train_net.py:76-87: resume from OUTPUT_DIR's last checkpoint, else initialise from MODEL.WEIGHT
    checkpointer = DetectronCheckpointer(
        cfg, model, optimizer, scheduler, cfg.OUTPUT_DIR if save_checkpoints else "", comm.get_rank() == 0,
        backbone_prefix=cfg.MODEL.BACKBONE_PREFIX,
        load_emb_pred_from=(cfg.MODEL.MMSS_HEAD.DEFAULT_HEAD if cfg.MODEL.LOAD_EMB_PRED_FROM_MMSS_HEAD else None),
        load_classifier=cfg.MODEL.LOAD_CLASSIFIER)
    resumed = checkpointer.has_checkpoint()
    extra = checkpointer.load(cfg.MODEL.WEIGHT, load_trainer_state=cfg.MODEL.LOAD_TRAINER_STATE)
    start_iter = int(extra.get("iteration", 0)) if cfg.MODEL.LOAD_TRAINER_STATE else 0
    if resumed and hasattr(model, "roi_heads_student") and not cfg.MODEL.RESUME:
        # st_generalized_rcnn.py:197-200 copies the teacher heads over the student at iteration 0 unless MODEL.RESUME
        logging.getLogger("ovis.trainer").warning(
            "resuming from %s with MODEL.RESUME False: the student heads in the checkpoint will be overwritten by the "
            "teacher's at the first iteration (set MODEL.RESUME True to keep them)", cfg.OUTPUT_DIR)
    if distributed:
        comm.broadcast_parameters(model)
    ema = None
    if ema_decay is not None:  # behind the checkpoint load (and the broadcast: every rank's average starts equal)
        ema = ModelEma(model, ema_decay)
        if cfg.MODEL.LOAD_TRAINER_STATE and "ema" in extra:
            ema.load_state_dict(extra["ema"])
        else:
            logging.getLogger("ovis.trainer").info("--ema %s: no average restored, it starts from the loaded weights "
                                                   "(%d tensors, update count 0)", ema_decay, len(ema.tensors))

    # host batches come from DATALOADER.NUM_WORKERS worker processes (the training process' interpreter lock is busy feeding
    # two HIP streams) and are staged through pinned memory on a copy stream, two batches ahead
    # --raw-input: the workers hand over raw uint8 images at their own sizes with polygon ground truth and only decide the
    # size and the flips (data/transforms.py); resize, flip, normalisation and padding run on the device behind the copy
    loader, transform = make_data_source(cfg, ims_per_gpu, raw_input, dataset, start_iter, max_iter, seed, color_jitter,
                                         scale_jitter, crop_size, copy_paste)
    data = DevicePrefetcher(loader, device, depth=2, transform=transform)
    if not cfg.MODEL.WEIGHT and not checkpointer.has_checkpoint():  # random init only: give the frozen BN usable statistics
        images, _ = make_batch(1, device=device, seed=7)
        calibrate_stem_bn(model, images)
    evaluator = None
    if evaluate:
        logger = logging.getLogger("ovis.trainer")
        if not cfg.SOLVER.SKIP_VAL_LOSS:
            logger.info("SOLVER.SKIP_VAL_LOSS False: the validation loss is not computed, --evaluate scores AP only")
        evaluator = functools.partial(evaluation.evaluate_in_training, cfg, model, catalog, device,
                                      train_class_embeddings=e_seen, logger=logger, boundary_ap=boundary_ap,
                                      lvis=lvis)
        if ema is not None:  # the periodic scoring sees the averaged weights and says so in where it writes
            scoring = functools.partial(evaluator, folder="inference_ema")

            def evaluator(iteration):
                with ema.applied(model):
                    return scoring(iteration)
    try:
        history = trainer.do_train(cfg, model, data, optimizer, scheduler, max_iter, start_iter=start_iter,
                                   checkpointer=checkpointer if save_checkpoints else None,
                                   checkpoint_period=cfg.SOLVER.CHECKPOINT_PERIOD, evaluator=evaluator,
                                   test_period=cfg.SOLVER.TEST_PERIOD if evaluate else 0,
                                   **({"ema": ema} if ema is not None else {}))
    finally:
        data.close()
    if evaluate and not skip_test:  # tools/train_net.py:129-159: the final test, the route of tools/infer_net.py --evaluate
        comm.synchronize()
        evaluation.run_datasets(cfg, model, catalog, device, logging.getLogger("ovis.inference"), evaluate=True,
                                boundary_ap=boundary_ap, lvis=lvis)
        comm.synchronize()
        if ema is not None:  # ... and once more on the averaged weights
            with ema.applied(model):
                evaluation.run_datasets(cfg, model, catalog, device, logging.getLogger("ovis.inference"), evaluate=True,
                                        boundary_ap=boundary_ap, lvis=lvis, folder="inference_ema")
            comm.synchronize()
    return history


def main(argv=None):
    parser = argparse.ArgumentParser(description="MI355X-native detection training (synthetic data)")
    parser.add_argument("--config-file", default="", metavar="FILE", help="path to config file")
    parser.add_argument("--local_rank", type=int, default=int(os.environ.get("LOCAL_RANK", 0)))
    parser.add_argument("--skip-test", dest="skip_test", action="store_true",
                        help="with --evaluate: do not run the final test behind the last iteration")
    parser.add_argument("--evaluate", action="store_true",
                        help="score every DATASETS.TEST set on the device behind every SOLVER.TEST_PERIOD-th iteration (COCO box / "
                             "mask AP, AP50 per class and split -> OUTPUT_DIR/inference/<name>/coco_results_<iteration>.json) and "
                             "run the final test behind the last one (predictions.pth, coco_results.json); needs "
                             "--dataset-catalog, OUTPUT_DIR and MODEL.DEVICE cuda")
    parser.add_argument("--boundary-ap", action="store_true",
                        help="with --evaluate and MODEL.MASK_ON: also score Boundary AP (Cheng et al., CVPR 2021) -- a boundary "
                             "task behind segm in every logged table and coco_results*.json, periodic and final")
    parser.add_argument("--lvis", action="store_true",
                        help="with --evaluate: score under LVIS-style federated rules (neg_category_ids, "
                             "not_exhaustive_category_ids, frequency: AP ... APl, APr, APc, APf; 300 detections per image) and "
                             "write lvis_results*.json in place of coco_results*.json")
    parser.add_argument("--max-iter", type=int, default=None, help="override SOLVER.MAX_ITER for a short run")
    parser.add_argument("--no-checkpoints", action="store_true",
                        help="do not write model_<iter>.pth / model_final.pth / last_checkpoint under OUTPUT_DIR and do not "
                             "resume from them (the reference always does both, tools/train_net.py:76-88)")
    parser.add_argument("--save-checkpoints", action="store_true", help="accepted for compatibility: saving is the default")
    parser.add_argument("--raw-input", action="store_true",
                        help="feed raw uint8 images at COCO-like sizes with polygon ground truth through the device input "
                             "transform (INPUT.* resize / flip / normalise, DATALOADER.SIZE_DIVISIBILITY) instead of "
                             "ready-made float32 800x1333 batches")
    parser.add_argument("--dataset-catalog", default=None, metavar="FILE",
                        help="JSON catalog {name: {img_dir, ann_file, ann_file_cap?, vocab_file?}}: train on DATASETS.TRAIN read "
                             "from these COCO-format files instead of the synthetic stream (implies --raw-input)")
    parser.add_argument("--color-jitter", action="store_true",
                        help="with --raw-input or --dataset-catalog: honour INPUT.BRIGHTNESS / CONTRAST / SATURATION / HUE -- "
                             "ColorJitter in front of the resize, drawn per image in the loader and run on the device (on the "
                             "host with MODEL.DEVICE cpu) with the bytes PIL produces; without the flag non-zero keys raise")
    parser.add_argument("--scale-jitter", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                        help="with --raw-input or --dataset-catalog: large-scale jitter -- per image a scale drawn from [LO, HI] "
                             "of the canvas in place of INPUT.MIN_SIZE_TRAIN, then a random crop or a zero pad to the canvas "
                             "(Detectron2's ResizeScale + FixedSizeCrop restated); boxes, polygon and RLE masks follow the crop. "
                             "Captions are carried unchanged: a crop can remove the object a caption noun names (HI <= 1 never "
                             "crops an image of the canvas' aspect ratio)")
    parser.add_argument("--crop-size", type=int, nargs=2, default=None, metavar=("H", "W"),
                        help="with --scale-jitter: the canvas every training image is cropped or padded to (default 1024 1024)")
    parser.add_argument("--copy-paste", type=float, default=None, metavar="P",
                        help="with --scale-jitter, MODEL.MASK_ON True and MODEL.DEVICE cuda: copy-paste augmentation between the "
                             "images of a batch -- image i receives, with probability P in (0, 1], each instance of image "
                             "(i + 1) %% B with probability 0.5, pasted at the same canvas position; covered masks lose the "
                             "occluded part, their boxes are recomputed, and instances left without extent are dropped.  Polygon "
                             "ground truth only.  Captions are carried unchanged: a pasted object is not named by the "
                             "destination's caption, and a covered one may still be named")
    parser.add_argument("--ema", type=float, default=None, metavar="DECAY",
                        help="keep an exponential moving average of the trainable weights, DECAY a float in (0, 1): moved "
                             "inside the fused SGD launch at every optimizer step with d_t = min(DECAY, (1 + t) / (10 + t)), "
                             "saved as the checkpoints' \"ema\" entry and restored on resume; with --evaluate the periodic "
                             "scoring and a second final test run on the averaged weights and write under "
                             "OUTPUT_DIR/inference_ema/ (inference/ always holds the raw weights' results)")
    parser.add_argument("--data-dir", default="", help="where the catalog's relative paths are taken from")
    parser.add_argument("--seed", type=int, default=0,
                        help="with --dataset-catalog: the run's seed of the input transform's random draws (sizes, flips)")
    parser.add_argument("opts", default=None, nargs=argparse.REMAINDER, help="KEY VALUE overrides")
    args = parser.parse_args(argv)

    num_gpus = int(os.environ.get("WORLD_SIZE", 1))
    distributed = num_gpus > 1
    cfg = get_defaults()
    if args.config_file:
        cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(args.opts or [])
    cfg.freeze()
    if args.ema is not None and not 0.0 < args.ema < 1.0:
        parser.error(f"--ema takes a decay in (0, 1), got {args.ema}")
    if args.evaluate and not args.dataset_catalog:
        parser.error("--evaluate runs the DATASETS.TEST sets of the catalog through the model: give --dataset-catalog")
    if args.evaluate and not cfg.OUTPUT_DIR:
        parser.error("--evaluate writes OUTPUT_DIR/inference/<name>/coco_results_<iteration>.json: set OUTPUT_DIR")
    if args.evaluate and cfg.MODEL.DEVICE != "cuda":
        parser.error("--evaluate scores on the HIP device (mask IoU and matching have no host implementation): "
                     "set MODEL.DEVICE cuda")
    if args.lvis and not args.evaluate:
        parser.error("--lvis changes the rules of what --evaluate scores: it is valid only with --evaluate")
    if args.boundary_ap and not args.evaluate:
        parser.error("--boundary-ap adds the boundary task to what --evaluate scores: give --evaluate too")
    if args.boundary_ap and not cfg.MODEL.MASK_ON:
        parser.error("--boundary-ap scores the mask head's masks: set MODEL.MASK_ON True")
    if args.evaluate and cfg.TEST.BBOX_AUG.ENABLED:
        parser.error("--evaluate scores one view per image while training: set TEST.BBOX_AUG.ENABLED False "
                     "(tools/infer_net.py runs multi-scale / flip testing on a checkpoint)")
    if args.color_jitter and not (args.raw_input or args.dataset_catalog):
        parser.error("--color-jitter acts on raw uint8 images in front of the device input transform: give --raw-input or "
                     "--dataset-catalog (the float32 synthetic stream has no bytes to jitter)")
    if args.color_jitter:
        try:
            check_color_jitter(getattr(cfg.INPUT, k) for k in JITTER_KEYS)
        except ValueError as e:
            parser.error(f"--color-jitter: {e}")
    if args.crop_size is not None and args.scale_jitter is None:
        parser.error("--crop-size is the canvas of --scale-jitter: give --scale-jitter LO HI too")
    if args.scale_jitter is not None and not (args.raw_input or args.dataset_catalog):
        parser.error("--scale-jitter acts in the device input transform: give --raw-input or --dataset-catalog (the float32 "
                     "synthetic stream has no bytes to resample)")
    if args.scale_jitter is not None:
        try:
            check_scale_jitter(args.scale_jitter, args.crop_size)
        except ValueError as e:
            parser.error(f"{'--crop-size' if str(e).startswith('crop_size') else '--scale-jitter'}: {e}")
    if args.copy_paste is not None:
        if args.scale_jitter is None:
            parser.error("--copy-paste pastes at the same position of the fixed canvas of --scale-jitter: give --scale-jitter "
                         "LO HI too")
        try:
            check_copy_paste(args.copy_paste)
        except ValueError as e:
            parser.error(f"--copy-paste: {e}")
        if cfg.MODEL.DEVICE != "cuda":
            parser.error("--copy-paste composites masks and pixels on the HIP device: set MODEL.DEVICE cuda")
        if not cfg.MODEL.MASK_ON:
            parser.error("--copy-paste edits the ground-truth masks: set MODEL.MASK_ON True")
    if cfg.MODEL.DEVICE == "cuda":
        torch.cuda.set_device(args.local_rank)
        # The training process does almost no CPU math, but every multi-threaded host op (a staging memcpy, a reduction over a
        # host tensor) wakes an OpenMP team as wide as the machine whose threads then SPIN for their blocktime -- on a
        # 256-thread host that starved the data-loader workers: next(loader) 31 instead of 6 ms per 2-image batch, 58 instead
        # of 33 ms per iteration (tools/experiments/loader_consume_probe.py).  A small team for the rank's core share.
        if "OMP_NUM_THREADS" not in os.environ:
            torch.set_num_threads(max(1, min(8, len(os.sched_getaffinity(0)) // 4)))
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl" if cfg.MODEL.DEVICE == "cuda" else "gloo", init_method="env://")
        comm.synchronize()
    logging.basicConfig(level=logging.INFO if comm.get_rank() == 0 else logging.WARNING,
                        format="%(asctime)s %(name)s %(levelname)s: %(message)s")
    logging.getLogger("ovis.trainer").info("Using %d GPUs\n%s", num_gpus, args)
    logging.getLogger("ovis.trainer").info("rank %d host cores: %s (%s)", comm.get_rank(), AFFINITY["cpus"], AFFINITY["source"])
    ims_per_gpu = max(cfg.SOLVER.IMS_PER_BATCH // num_gpus, 1)
    logging.getLogger("ovis.trainer").info("%d images per GPU and iteration (SOLVER.IMS_PER_BATCH %d / %d GPUs)", ims_per_gpu,
                                           cfg.SOLVER.IMS_PER_BATCH, num_gpus)
    train(cfg, args.local_rank, distributed, args.max_iter or cfg.SOLVER.MAX_ITER, ims_per_gpu,
          save_checkpoints=bool(cfg.OUTPUT_DIR) and not args.no_checkpoints, raw_input=args.raw_input,
          dataset_catalog=args.dataset_catalog, data_dir=args.data_dir, seed=args.seed, evaluate=args.evaluate,
          skip_test=args.skip_test, boundary_ap=args.boundary_ap, lvis=args.lvis, color_jitter=args.color_jitter,
          scale_jitter=args.scale_jitter, crop_size=args.crop_size, copy_paste=args.copy_paste,
          **({"ema_decay": args.ema} if args.ema is not None else {}))
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
