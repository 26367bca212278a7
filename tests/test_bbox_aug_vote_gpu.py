"""GPU: box voting and view-averaged masks through ``im_detect_bbox_aug`` on the tiny model: H_FLIP + two scales (four views,
the second mirrored).  Off means bit-identical to a call without the keywords; voting moves the boxes to the restatement's
(tests/box_vote_ref.py) within its bound and nothing else; averaged masks equal the float32 mean formed here from
``BoxList.resize`` / ``transpose``, ``model.segment`` per view and ``torch.flip``."""
import pytest
import torch

from tests import box_vote_ref as R
from tests.test_view_masks import expression

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import im_detect_bbox_aug
    from tests.tiny_model import build_tiny

    model, _, e_seen, _, _ = build_tiny("student_teacher_mask_rcnn_uncertainty")
    model = model.cuda()
    model.set_class_embeddings(e_seen.cuda())
    model.eval()
    cfg = get_defaults()
    cfg.merge_from_list(["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (64, 96),
                         "TEST.BBOX_AUG.MAX_SIZE", 160, "INPUT.MIN_SIZE_TEST", 80, "INPUT.MAX_SIZE_TEST", 128])
    transform = build_transforms(cfg, is_train=False)
    g = torch.Generator().manual_seed(3)
    raw, _ = transform.host([torch.randint(0, 256, (61, 83, 3), dtype=torch.uint8, generator=g),
                             torch.randint(0, 256, (90, 57, 3), dtype=torch.uint8, generator=g)])
    batch = transform.device({k: v.cuda() if torch.is_tensor(v) else v for k, v in raw.items()})
    assert len(batch) == 4 and batch.flips == [False, True, False, False]
    plain = im_detect_bbox_aug(model, batch)          # computed once, shared, never written to
    assert sum(len(p) for p in plain) > 0 and all("mask" in p.fields() for p in plain)
    return model, batch, plain


def _same_boxlists(got, want, but=()):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.size == w.size and sorted(g.fields()) == sorted(w.fields())
        if "bbox" not in but:
            assert torch.equal(g.bbox, w.bbox)
        for f in w.fields():
            if f not in but:
                assert g.get_field(f).dtype == w.get_field(f).dtype and torch.equal(g.get_field(f), w.get_field(f)), f


def test_both_options_off_is_the_call_without_them(tiny):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import im_detect_bbox_aug

    model, batch, plain = tiny
    _same_boxlists(im_detect_bbox_aug(model, batch, vote_thresh=None, average_masks=False), plain)
    _same_boxlists(im_detect_bbox_aug(model, batch, None, None, False), plain)


def _merged_and_kept(model, batch):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import NMS_SLICE_CANDIDATES, view_segments

    per_view = [model.detect_unfiltered(images)[1] for images in batch.views]
    nc = model.roi_heads["box"].predictor.num_classes
    post = model.roi_heads_student["box"].post_processor
    merged = _C.merge_view_detections(*view_segments(per_view, batch.flips, nc), nc, post.score_thresh)
    _, kept = post.filter_merged(merged, [d.size for d in per_view[0]], nc, slice_candidates=NMS_SLICE_CANDIDATES,
                                 return_kept=True)
    return merged, torch.cat(kept), per_view


def test_voting_moves_the_boxes_to_the_restatement_and_nothing_else(tiny):
    """Raises TypeError without the feature: ``im_detect_bbox_aug`` has no ``vote_thresh``."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import im_detect_bbox_aug

    model, batch, plain = tiny
    voted = im_detect_bbox_aug(model, batch, vote_thresh=0.5)
    maps = tuple(f for f in plain[0].fields() if f not in ("scores", "labels"))             # taken on the voted boxes
    _same_boxlists(voted, plain, but=("bbox",) + maps)                                      # labels, scores, counts, order
    for v, p in zip(voted, plain):
        assert len(v) == len(p) and torch.equal(v.get_field("scores"), p.get_field("scores"))
        assert torch.equal(v.get_field("labels"), p.get_field("labels"))
    merged, kept, _ = _merged_and_kept(model, batch)
    cand_boxes, cand_scores, cand_group, offsets = (t.cpu().numpy() for t in merged)
    assert torch.equal(merged[0][kept], torch.cat([p.bbox for p in plain]))                 # kept = the plain detections
    want, n = R.vote(cand_boxes, cand_scores, offsets, cand_group, kept.cpu().numpy(), 0.5)
    assert n.max() > 1                                                                      # some box did move
    R.assert_within_bound(torch.cat([v.bbox for v in voted]).cpu().numpy(), want, n)
    assert not torch.equal(torch.cat([v.bbox for v in voted]), torch.cat([p.bbox for p in plain]))


def test_averaged_masks_are_the_mean_over_the_views(tiny):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import im_detect_bbox_aug

    model, batch, plain = tiny
    got = im_detect_bbox_aug(model, batch, average_masks=True)
    _same_boxlists(got, plain, but=("mask",))                      # boxes, scores, labels and every other map: view 0's
    boxes = [p.copy_with_fields(["scores", "labels"]) for p in plain]
    maps = []
    for images, flip in zip(batch.views, batch.flips):
        features, detections = model.detect_unfiltered(images)
        there = [b.resize(d.size) for b, d in zip(boxes, detections)]
        there = [b.transpose(0) for b in there] if flip else there
        maps.append([m.get_field("mask") for m in model.segment(features, there)])
    moved = 0
    for i, g in enumerate(got):
        want = expression(torch.stack([m[i].cpu() for m in maps]), batch.flips)
        assert torch.equal(g.get_field("mask").cpu(), want)
        assert torch.equal(maps[0][i], plain[i].get_field("mask"))
        moved += int(not torch.equal(g.get_field("mask"), plain[i].get_field("mask")))
    assert moved > 0
    with pytest.raises(ValueError, match=r"\(0, 1\]"):
        im_detect_bbox_aug(model, batch, vote_thresh=1.5)


def test_both_options_together(tiny):
    """The masks are taken on the VOTED boxes."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import im_detect_bbox_aug

    model, batch, _ = tiny
    voted = im_detect_bbox_aug(model, batch, vote_thresh=0.5)
    both = im_detect_bbox_aug(model, batch, vote_thresh=0.5, average_masks=True)
    _same_boxlists(both, voted, but=("mask",))
    boxes = [v.copy_with_fields(["scores", "labels"]) for v in voted]
    maps = []
    for images, flip in zip(batch.views, batch.flips):
        features, detections = model.detect_unfiltered(images)
        there = [b.resize(d.size) for b, d in zip(boxes, detections)]
        there = [b.transpose(0) for b in there] if flip else there
        maps.append(torch.cat([m.get_field("mask") for m in model.segment(features, there)]).cpu())
    assert torch.equal(torch.cat([b.get_field("mask") for b in both]).cpu(), expression(torch.stack(maps), batch.flips))
