"""Score COCO results files against an annotation file on the device: COCO box / mask AP and the per-class / per-split AP50
of ``bbox.json`` / ``segm.json`` -- the files ``tools/infer_net.py --export-results`` writes, or those of the reference
(maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py: ``do_coco_evaluation`` :40-61), or of any other tool --
without a model, a configuration or the images (engine/coco_eval.py: ``evaluate_coco_results``).  The RLE masks of
``segm.json`` are decoded on the device straight to the scorer's bit words (csrc/coco_rle_decode.hip).

  python tools/score_results.py --ann-file instances_val.json --results-dir OUTPUT_DIR/inference/<name>
  python tools/score_results.py --ann-file instances_val.json --segm segm.json --output scores.json
  python tools/score_results.py --ann-file instances_val.json --segm segm.json --boundary-ap
  python tools/score_results.py --ann-file lvis_v1_val.json --results-dir DIR --lvis --boundary-ap --recall

Prints the ``Task: ... / names / values`` table ``--evaluate`` logs; ``--output`` writes the numbers as
``coco_results.json`` has them.  ``--recall`` adds COCO's AR numbers behind the AP keys, from the same match tables.  ``--boundary-ap`` adds a ``boundary`` task
behind ``segm``: Boundary AP (Cheng et al., CVPR 2021) of the same ``segm.json`` -- segm's keys from a matching on min(mask IoU,
boundary IoU), the rule as include/ovis_hip.h states it (not compared with boundary-iou-api's output); the masks are decoded
once for both.  ``--lvis`` scores every task under LVIS-style federated rules instead -- AP ... APl, APr, APc, APf, with
``--recall`` AR@300 ...; the annotation file must carry ``neg_category_ids``, ``not_exhaustive_category_ids`` and ``frequency``
(the ten rules of include/ovis_hip.h; not compared with lvis-api's output).  ``--error-analysis`` (not with ``--lvis``) breaks AP50
down by error type from the same scoring pass (engine/error_analysis.py: Cls, Loc, Both, Dupe, Bkg, Miss and the AP50 each
would give back, per split; the rules of include/ovis_hip.h, not compared with tidecv's output): ``errors_bbox`` /
``errors_segm`` tables behind the others and, with the counts, under those names in ``--output``.  There is no host-only scoring: the device must be a HIP device.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IOU_TYPES = ("bbox", "segm")  # the results files there are; --boundary-ap scores segm.json a second way


def main(argv=None):
    parser = argparse.ArgumentParser(description="Score COCO results files (bbox.json / segm.json) on the device")
    parser.add_argument("--ann-file", required=True, metavar="FILE", help="the COCO annotation file the results belong to")
    parser.add_argument("--bbox", default=None, metavar="PATH", help="a bbox results file")
    parser.add_argument("--segm", default=None, metavar="PATH", help="a segm results file (RLE masks)")
    parser.add_argument("--results-dir", default=None, metavar="DIR", help="DIR/bbox.json and DIR/segm.json, whichever exist")
    parser.add_argument("--output", default=None, metavar="PATH", help="write {iou_type: {metric: value}} as JSON")
    parser.add_argument("--recall", action="store_true",
                        help="add COCO's AR1 / AR10 / AR100 / ARs / ARm / ARl and AR100 per split behind the AP keys (results "
                             "files are capped per category, so they are not proposal lists: no box_proposal task)")
    parser.add_argument("--boundary-ap", action="store_true",
                        help="also score Boundary AP (Cheng et al., CVPR 2021) from the segm results file: a boundary task "
                             "behind segm -- segm's keys, matched on min(mask IoU, boundary IoU)")
    parser.add_argument("--lvis", action="store_true",
                        help="LVIS-style federated rules: the annotation file's neg_category_ids / "
                             "not_exhaustive_category_ids / frequency decide what is judged; 300 detections per image; adds "
                             "APr / APc / APf (with --recall: AR@300, ARs@300, ARm@300, ARl@300)")
    parser.add_argument("--error-analysis", action="store_true",
                        help="break AP50 down by error type (Cls, Loc, Both, Dupe, Bkg, Miss; dAP50 per type and split): "
                             "errors_bbox / errors_segm tasks behind the others, in --output too; not with --lvis")
    parser.add_argument("--device", default="cuda", help="the HIP device that scores (cuda, cuda:1, ...)")
    args = parser.parse_args(argv)
    files = {}
    for iou_type in IOU_TYPES:
        path = getattr(args, iou_type)
        if path is None and args.results_dir and os.path.exists(os.path.join(args.results_dir, iou_type + ".json")):
            path = os.path.join(args.results_dir, iou_type + ".json")
        if path is not None:
            files[iou_type] = path
    if not files:
        parser.error("no results file: give --bbox, --segm or a --results-dir that holds bbox.json or segm.json")
    if args.error_analysis and args.lvis:
        parser.error("--error-analysis follows COCO's rules: it does not go with --lvis (under federated annotation an "
                     "unannotated object makes the background error meaningless)")
    if args.boundary_ap and "segm" not in files:
        parser.error("--boundary-ap scores the masks of a segm results file: give --segm or a --results-dir that holds "
                     "segm.json")
    for path in [args.ann_file] + list(files.values()):
        if not os.path.exists(path):
            parser.error(f"{path} does not exist")
    try:
        device = torch.device(args.device)
    except RuntimeError:
        parser.error(f"--device {args.device} is not a device")
    if device.type != "cuda" or not torch.cuda.is_available():
        parser.error("results are scored on the HIP device (mask decoding, IoU and matching have no host implementation): "
                     "--device cuda on a machine that has one")

    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval, error_analysis

    dataset = coco_eval.annotation_dataset(args.ann_file)
    iou_types = IOU_TYPES + (("boundary",) if args.boundary_ap else ())
    scored = {}
    extra = {"rules": "lvis"} if args.lvis else {}
    if args.error_analysis:
        extra = {"error_thresholds": (error_analysis.FG_THRESHOLD, error_analysis.BG_THRESHOLD), "tables_out": scored}
    results = coco_eval.evaluate_coco_results(dataset, files, iou_types, device, recall=args.recall, **extra)
    print(coco_eval.format_results(results))
    if args.error_analysis:
        analysis = error_analysis.analyze_scored(dataset, scored, scored["cat_ids"])
        print(coco_eval.format_results(error_analysis.task_tables(analysis)))
        results.update((f"errors_{t}", numbers) for t, numbers in analysis.items())
    if args.output:
        with open(args.output, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
