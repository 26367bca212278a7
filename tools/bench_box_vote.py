"""A/B of the two options of multi-scale / flip testing on one MI355X (profiles/ab_box_vote.txt):

    python tools/bench_box_vote.py [--iters 20] [--pass-iters 3] [--parent-module FILE]

1. ``_C.vote_boxes`` against the same rule written with torch ops, on the merged candidate list of 2 images x 6 views x 1000
   proposals x 66 classes (the inputs of ``tools/bench_ops.py --ops view_merge``) and the detections ``filter_merged`` keeps.
2. The whole test-time-augmentation pass per batch (``im_detect_bbox_aug`` on two 480 x 640 images, six views: 800, 400 and
   1200 px, each plain and mirrored; the student-teacher mask configuration with random weights, region embeddings
   widened) with the options off, with voting, with view-averaged masks and with both.  ``--parent-module FILE``: an earlier revision of engine/bbox_aug.py,
   loaded beside the current one and timed in the same rounds (the options-off pass must not differ from it).

The variants alternate inside one process, three rounds each; device work is timed by a host clock around a synchronise.
One JSON line per measurement."""
import argparse
import importlib.util
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvpr22_cross_modal_pseudo_labeling_amd import _C  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.engine import bbox_aug  # noqa: E402

YAML = os.path.join(ROOT, "configs", "coco_cap_det", "student_teacher_mask_rcnn_uncertainty.yaml")


def timeit(fn, iters, warm=0.3):
    t0 = time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= warm:
            break
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def vote_by_tensor_ops(cand_boxes, cand_scores, cand_group, kept, thr):
    """The rule of ``_C.vote_boxes`` with torch ops: an IoU matrix [D, K] (structures.box_iou's expression), voters = same
    group and IoU >= thr, a matrix product for the weighted sums."""
    a, b = cand_boxes[kept], cand_boxes
    area_a = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    area_b = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    wh = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2]) + 1).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    iou = inter / (area_a[:, None] + area_b - inter)
    w = ((iou >= thr) & (cand_group[kept][:, None] == cand_group)).to(torch.float32) * cand_scores
    return (w @ cand_boxes) / w.sum(1, keepdim=True)


def bench_vote(args, dev):
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import PostProcessor

    g = torch.Generator().manual_seed(0)
    n_img, rows, nc = 2, 1000, 66
    views = [((1066, 800), 0), ((1066, 800), 1), ((533, 400), 0), ((533, 400), 1), ((1599, 1200), 0), ((1599, 1200), 1)]
    post = PostProcessor(get_defaults())
    boxes, scores, segments, row = [], [], [], 0
    for i in range(n_img):
        for (w, h), flip in views:
            xy = torch.rand(rows, nc, 2, generator=g) * torch.tensor([w * 0.7, h * 0.7])
            wh = torch.rand(rows, nc, 2, generator=g) * torch.tensor([w * 0.3, h * 0.3]) + 4
            boxes.append(torch.cat([xy, (xy + wh).clamp(max=min(w, h) - 1)], 2))
            scores.append(torch.softmax(torch.randn(rows, nc, generator=g) * 2.0, 1))
            segments.append((row, rows, i, w, flip, float(views[0][0][0]) / float(w), float(views[0][0][1]) / float(h)))
            row += rows
    merged = _C.merge_view_detections(torch.cat(boxes).to(dev), torch.cat(scores).to(dev), segments, nc, post.score_thresh)
    cand_boxes, cand_scores, cand_group, offsets = merged
    _, kept = post.filter_merged(merged, [views[0][0]] * n_img, nc, slice_candidates=bbox_aug.NMS_SLICE_CANDIDATES,
                                 return_kept=True)
    kept = torch.cat(kept)
    thr = 0.5

    def kernel():
        return _C.vote_boxes(cand_boxes, cand_scores, offsets, cand_group, kept, thr)

    def tensor_ops():
        return vote_by_tensor_ops(cand_boxes, cand_scores, cand_group, kept, thr)

    got, want = kernel().double(), tensor_ops().double()
    k_ms, t_ms = [], []
    for _ in range(3):
        k_ms.append(timeit(kernel, args.iters))
        t_ms.append(timeit(tensor_ops, args.iters))
    runs = (offsets[1:] - offsets[:-1])[cand_group[kept].long()]
    print(json.dumps({"op": "vote_boxes", "shape": f"{n_img} images x {len(views)} views x {rows} rows x {nc} classes",
                      "candidates": cand_boxes.shape[0], "detections": kept.numel(), "vote_thresh": thr,
                      "mean_run_of_a_detection": float(runs.float().mean()), "longest_run_of_a_detection": int(runs.max()),
                      "ms": sorted(k_ms)[1], "rounds_ms": [round(v, 4) for v in k_ms],
                      "tensor_ops_ms": sorted(t_ms)[1], "tensor_ops_rounds_ms": [round(v, 4) for v in t_ms],
                      "tensor_ops_over_kernel": sorted(t_ms)[1] / sorted(k_ms)[1],
                      "max_relative_difference": float(((got - want).abs() / want.abs().clamp(min=1.0)).max())}), flush=True)


def bench_pass(args, dev):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import calibrate_stem_bn, make_batch, make_embeddings
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.detector import build_detection_model

    cfg = get_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (400, 1200),
                         "TEST.BBOX_AUG.MAX_SIZE", 2000, "TEST.BBOX_AUG.SCALE_H_FLIP", True])
    cfg.freeze()
    torch.manual_seed(11)
    model = build_detection_model(cfg).to(dev)
    calibrate_stem_bn(model, make_batch(1, device=dev, seed=7)[0])
    model.set_class_embeddings(make_embeddings(cfg.MODEL.ROI_BOX_HEAD.EMB_DIM, device=dev)[1])
    with torch.no_grad():   # random-init region embeddings score every class alike (nothing passes SCORE_THRESH): widen them
        for heads in (model.roi_heads, model.roi_heads_student):
            heads["box"].predictor.emb_pred.weight.mul_(100.0)
    model.eval()
    transform = build_transforms(cfg, is_train=False)
    g = torch.Generator().manual_seed(5)
    raw, _ = transform.host([torch.randint(0, 256, (480, 640, 3), dtype=torch.uint8, generator=g) for _ in range(2)])
    batch = transform.device({k: v.to(dev) if torch.is_tensor(v) else v for k, v in raw.items()})
    variants = {"options_off": lambda: bbox_aug.im_detect_bbox_aug(model, batch),
                "vote_0.5": lambda: bbox_aug.im_detect_bbox_aug(model, batch, vote_thresh=0.5),
                "mask_aug": lambda: bbox_aug.im_detect_bbox_aug(model, batch, average_masks=True),
                "vote_0.5_and_mask_aug": lambda: bbox_aug.im_detect_bbox_aug(model, batch, vote_thresh=0.5, average_masks=True)}
    if args.parent_module:
        spec = importlib.util.spec_from_file_location(bbox_aug.__package__ + ".bbox_aug_parent", args.parent_module)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        variants = {"parent_revision": lambda: parent.im_detect_bbox_aug(model, batch), **variants}
        a, b = parent.im_detect_bbox_aug(model, batch), bbox_aug.im_detect_bbox_aug(model, batch)
        same = all(torch.equal(x.bbox, y.bbox) and all(torch.equal(x.get_field(f), y.get_field(f)) for f in x.fields())
                   for x, y in zip(a, b))
    else:
        same = None
    rounds = {name: [] for name in variants}
    for _ in range(3):
        for name, fn in variants.items():
            rounds[name].append(timeit(fn, args.pass_iters, warm=1.0))
    out = variants["options_off"]()
    per_view = [model.detect_unfiltered(images)[1] for images in batch.views]
    nc = model.roi_heads["box"].predictor.num_classes
    post = model.roi_heads_student["box"].post_processor
    merged = _C.merge_view_detections(*bbox_aug.view_segments(per_view, batch.flips, nc), nc, post.score_thresh)
    print(json.dumps({"op": "im_detect_bbox_aug", "views": [list(v.tensors.shape) for v in batch.views], "flips": batch.flips,
                      "candidates": merged[0].shape[0], "detections": [len(o) for o in out],
                      "options_off_equals_parent_revision": same,
                      "ms": {k: sorted(v)[1] for k, v in rounds.items()},
                      "rounds_ms": {k: [round(x, 2) for x in v] for k, v in rounds.items()}}), flush=True)


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--iters", type=int, default=20, help="timed calls per round of the voting A/B")
    parser.add_argument("--pass-iters", type=int, default=3, help="timed passes per round of the whole-pass A/B")
    parser.add_argument("--parent-module", default="", metavar="FILE", help="an earlier revision of engine/bbox_aug.py")
    parser.add_argument("--only", choices=("vote", "pass"), default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_vote.py measures on the HIP device: none found")
    dev = torch.device("cuda", 0)
    if args.only != "pass":
        bench_vote(args, dev)
    if args.only != "vote":
        bench_pass(args, dev)


if __name__ == "__main__":
    main()
