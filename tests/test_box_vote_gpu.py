"""GPU: the box-voting kernel (csrc/box_vote.hip through ``_C.vote_boxes``) on the case table of tests/box_vote_ref.py:
against the NumPy restatement within the bound derived there, the same bits on every call, the same bits as the host twin
(which keeps the wavefront's summation order), and the refusal of kept indices outside their run."""
import pytest
import torch

from tests import box_vote_ref as R

pytestmark = pytest.mark.gpu


def _tensors(name, device):
    return tuple(torch.from_numpy(a).to(device) for a in R.CASES[name][:5]) + (R.CASES[name][5],)


@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_within_the_bound_and_reproducible(name):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    want, n = R.want(name)
    got = _C.vote_boxes(*_tensors(name, "cuda"))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(n), 4)
    R.assert_within_bound(got.cpu().numpy(), want, n, name)
    again = _C.vote_boxes(*_tensors(name, "cuda"))
    assert torch.equal(got, again)                                        # no atomics: the same bits on every call
    # the host twin sums lane by lane and folds the lanes by the same butterfly: IEEE operations in one order, one result
    assert torch.equal(got.cpu(), _C.vote_boxes(*_tensors(name, "cpu")))


def test_more_detections_than_one_workgroup():
    """Every candidate of the lane-stride case as a kept detection (322 wavefronts, 81 workgroups, the last one partial)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    boxes, scores, offsets, group, _, thr = R.CASES["lane_stride_edges"]
    kept = torch.arange(boxes.shape[0], dtype=torch.int64)
    assert kept.numel() % 4 != 0
    want, n = R.vote(boxes, scores, offsets, group, kept.numpy(), thr)
    got = _C.vote_boxes(*(torch.from_numpy(a).cuda() for a in (boxes, scores, offsets, group)), kept.cuda(), thr)
    R.assert_within_bound(got.cpu().numpy(), want, n)


def test_bad_kept_indices_raise_on_the_device():
    """The kernel forms no address from a kept index before it has been checked against K, the group count and the run
    (csrc/box_vote.hip); what it refuses comes back as a status."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    boxes, scores, offsets, group, _, thr = _tensors("two_images_three_classes", "cuda")
    k = boxes.shape[0]
    for bad in ([k], [-1], [0, k + 5]):
        with pytest.raises(RuntimeError, match="kept index"):
            _C.vote_boxes(boxes, scores, offsets, group, torch.tensor(bad, dtype=torch.int64, device="cuda"), thr)
    moved = group.clone()
    moved[0] = 4                                  # candidate 0 claims a group whose run is [3, 5)
    with pytest.raises(RuntimeError, match="kept index"):
        _C.vote_boxes(boxes, scores, offsets, moved, torch.tensor([0], dtype=torch.int64, device="cuda"), thr)
    moved[0] = 17                                 # ... and a group that does not exist
    with pytest.raises(RuntimeError, match="kept index"):
        _C.vote_boxes(boxes, scores, offsets, moved, torch.tensor([0], dtype=torch.int64, device="cuda"), thr)
    with pytest.raises(RuntimeError, match="mixed"):
        _C.vote_boxes(boxes, scores, offsets, group, torch.tensor([0], dtype=torch.int64), thr)


def test_filter_merged_returns_the_kept_candidates_on_the_device():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import PostProcessor

    g = torch.Generator().manual_seed(9)
    n, nc, views, images = 40, 7, 3, 2
    r = n * views * images
    xy = torch.rand(r, nc, 2, generator=g) * 300
    boxes = torch.cat([xy, xy + torch.rand(r, nc, 2, generator=g) * 150 + 10], 2)
    scores = torch.softmax(torch.randn(r, nc, generator=g) * 3.0, 1)
    segments = [(k * n, n, k // views, 501, k % 2, 1.0, 1.0) for k in range(views * images)]
    host = _C.merge_view_detections(boxes, scores, segments, nc, 0.05)
    merged = tuple(t.cuda() for t in host)
    sizes = [(501, 375)] * images
    pp = PostProcessor(get_defaults())
    for per_img, slices in ((100, None), (5, None), (100, 64)):     # under / over the DETECTIONS_PER_IMG cut, sliced NMS
        pp.detections_per_img = per_img
        plain = pp.filter_merged(merged, sizes, nc, slice_candidates=slices)
        results, kept = pp.filter_merged(merged, sizes, nc, slice_candidates=slices, return_kept=True)
        _, host_kept = pp.filter_merged(host, sizes, nc, return_kept=True)
        for p, q, idx, h in zip(plain, results, kept, host_kept):
            assert torch.equal(p.bbox, q.bbox) and torch.equal(p.get_field("scores"), q.get_field("scores"))
            assert idx.dtype == torch.int64 and idx.is_cuda and torch.equal(merged[0][idx], q.bbox)
            assert torch.equal(idx.cpu(), h)
