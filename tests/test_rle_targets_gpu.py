"""GPU: mask targets from RLE ground truth.  ``_C.project_rle_masks`` (csrc/rle_targets.hip) must equal, bit for bit, the
dense NumPy restatement of its chain (tests/rle_targets_reference.py, itself held to the reference by
tests/test_rle_targets_reference.py); the decode without host reads (``_C.coco_rle_words_staged``) must give what
``_C.coco_rle_words`` gives; and a training step of the tiny model runs from an RLE annotation file through the loader, the
prefetcher and the device half of the input transform, with a malformed encoding reported one batch late at most."""
import copy

import numpy as np
import pytest
import torch

from tests import coco_rle_reference as rle_ref
from tests import rle_targets_reference as rt
from tests import tiny_coco, tiny_rle_coco

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 3


def _rle_masks(bitmaps, **kw):
    """RleMasks of bool [G, h, w] bitmaps: compressed strings and uncompressed lists alternate."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import RleMasks

    items = [rle_ref.rle_to_string(rle_ref.rle_encode(m)).decode("ascii") if k % 2 == 0 else rle_ref.rle_encode(m)
             for k, m in enumerate(bitmaps)]
    return RleMasks(items, bitmaps.shape[1:], **kw)


@pytest.fixture(scope="module")
def sources():
    """{shape index: (bool [G, h0, w0] salt-and-pepper bitmaps, their decoded RleMasks on the device)} -- decoded once."""
    out = {}
    for s, ((h0, w0), _) in enumerate(rt.SHAPES):
        bitmaps = rt.salt_and_pepper(G, h0, w0, 40 + s)
        out[s] = (bitmaps, _rle_masks(bitmaps).to(DEV).decoded())
    return out


# w0 = 50 and 45: rows straddle words; 48 x 64 is a multiple of 64 pixels, the others are not
@pytest.mark.parametrize("M", [14, 28])
@pytest.mark.parametrize("s", range(len(rt.SHAPES)), ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in rt.SHAPES])
def test_kernel_equals_the_restatement(sources, s, M):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    (h0, w0), (h1, w1) = rt.SHAPES[s]
    bitmaps, decoded = sources[s]
    assert decoded.words.is_cuda and decoded.word_offsets.tolist() == [k * ((h0 * w0 + 63) // 64) for k in range(G + 1)]
    boxes = np.concatenate([rt.edge_boxes(w1, h1), rt.random_boxes(10, w1, h1, 7 + s)])
    gt_index = np.arange(len(boxes)) % G   # spread over the instances
    keep = torch.tensor([True, False, True])
    sub_index = np.arange(len(boxes)) % 2
    boxes_dev = torch.from_numpy(boxes).to(DEV)
    for flip_h, flip_v in rt.FLIPS:
        m = decoded.resize((w1, h1))
        m = m.transpose(0) if flip_h else m
        m = m.transpose(1) if flip_v else m
        got = _C.project_rle_masks(m, torch.from_numpy(gt_index).to(DEV), boxes_dev, M)
        want = rt.project(bitmaps, gt_index, boxes, (h1, w1), flip_h, flip_v, M)
        assert got.shape == (len(boxes), M, M) and got.dtype == torch.float32
        differ = (got.cpu().numpy() != want)
        assert not differ.any(), (flip_h, flip_v, int(differ.sum()), np.argwhere(differ)[:5].tolist())
        assert 0 < want.mean() < 1
        # an indexed subset: instances 0 and 2, nothing repacked
        sub = m[keep.to(DEV)]
        assert sub.words is m.words and sub.instance.tolist() == [0, 2]
        got = _C.project_rle_masks(sub, torch.from_numpy(sub_index).to(DEV), boxes_dev, M)
        want = rt.project(bitmaps[[0, 2]], sub_index, boxes, (h1, w1), flip_h, flip_v, M)
        assert np.array_equal(got.cpu().numpy(), want), (flip_h, flip_v, "subset")
    empty = _C.project_rle_masks(m, torch.zeros(0, dtype=torch.int64, device=DEV), boxes_dev[:0], M)
    assert empty.shape == (0, M, M) and empty.is_cuda


def test_sizes_the_kernel_does_not_take_are_refused(sources):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    _, decoded = sources[0]
    boxes = torch.tensor([[1.0, 1.0, 20.0, 20.0]], device=DEV)
    idx = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="OVIS_ERANGE"):
        _C.project_rle_masks(decoded, idx, boxes, 129)   # the tap tables hold 128 rows
    wrong = decoded._with(source_hw=(37, 64))   # a slice's word count no longer matches h0 x w0
    with pytest.raises(RuntimeError, match="OVIS_ERANGE"):
        _C.project_rle_masks(wrong, idx, boxes, 14)


def _staged(items, sizes):
    """``_C.coco_rle_words_staged`` on ``items`` packed by the host form of RleMasks, with the host's word offsets."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import RleMasks

    packed = RleMasks(items, (1, 1)).to(DEV)   # the packing does not depend on the size
    per_mask = [(h * w + 63) // 64 if h >= 1 and w >= 1 and h * w <= 0x7fffffef else 0 for h, w in sizes]
    offsets = np.concatenate([[0], np.cumsum(per_mask)]).astype(np.int64)
    words, areas, status = _C.coco_rle_words_staged(
        packed.chars, packed.char_offsets, packed.runs, packed.run_offsets, torch.tensor(sizes, dtype=torch.int32, device=DEV),
        torch.from_numpy(offsets).to(DEV), total_words=int(offsets[-1]), max_words=max(per_mask), compressed=packed.num_chars > 0)
    return words, torch.from_numpy(offsets), areas, status


def test_decode_without_host_reads_equals_coco_rle_words():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C, _lib

    noise = np.random.default_rng(1).random((37, 53)) > 0.5
    runs = rle_ref.rle_encode(noise)
    text = rle_ref.rle_to_string(runs).decode("ascii")
    small = np.zeros((5, 7), dtype=bool)
    small[4, 6] = True
    small_text = rle_ref.rle_to_string(rle_ref.rle_encode(small)).decode("ascii")
    mid = len(text) // 2
    short, long_ = list(runs), list(runs)
    short[-1] -= 1
    long_[-1] += 1
    malformed = [(text[:mid] + "p" + text[mid + 1:], [37, 53], _lib.OVIS_COCO_RLE_BAD_CHAR),
                 (text + "P", [37, 53], _lib.OVIS_COCO_RLE_UNTERMINATED),
                 (rle_ref.rle_to_string(short).decode("ascii"), [37, 53], _lib.OVIS_COCO_RLE_BAD_SUM),
                 (long_, [37, 53], _lib.OVIS_COCO_RLE_BAD_SUM),
                 ([10, -3, 28], [5, 7], _lib.OVIS_COCO_RLE_NEGATIVE_RUN),
                 ("5" + "o" * 9 + "0", [5, 7], _lib.OVIS_COCO_RLE_OVERFLOW),
                 ([0], [0, 5], _lib.OVIS_COCO_RLE_BAD_SIZE)]
    calls = [([text, small_text, text], [[37, 53], [5, 7], [37, 53]], [0, 0, 0]),       # compressed items
             ([runs, rle_ref.rle_encode(small)], [[37, 53], [5, 7]], [0, 0]),           # list items
             ([small_text, runs, text, rle_ref.rle_encode(small)], [[5, 7], [37, 53], [37, 53], [5, 7]], [0] * 4)]   # mixed
    calls += [([small_text, item, runs], [[5, 7], size, [37, 53]], [0, code, 0]) for item, size, code in malformed]
    for items, sizes, codes in calls:
        want = _C.coco_rle_words(items, torch.tensor(sizes, dtype=torch.int32, device=DEV))
        words, offsets, areas, status = _staged(items, sizes)
        assert status.tolist() == codes == want[3].tolist(), (sizes, status.tolist())
        assert offsets.tolist() == want[1].tolist() and torch.equal(words, want[0]) and torch.equal(areas, want[2])
    assert int(_staged([text], [[37, 53]])[2][0]) == int(noise.sum())


def test_batch_decode_and_projection_make_no_host_round_trip():
    """The device half of the input transform decodes the RleMasks of a batch -- two images of different sizes, strings and
    lists -- in one call, and the mask loss' projection follows, with torch's synchronisation check set to 'error': no
    device-to-host copy, no blocking host-to-device copy.  The status is looked at afterwards (``flush``)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import InputTransform
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList

    transform = InputTransform((64,), 128, 0.0, 0.0, [0.0] * 3, [1.0] * 3, True)
    bitmaps = [rt.salt_and_pepper(2, 37, 50, 70), rt.salt_and_pepper(3, 61, 45, 71)]
    boxes = [torch.tensor([[2.0, 3.0, 30.0, 20.0], [0.0, 0.0, 39.0, 20.0]]), torch.tensor([[5.5, 6.5, 80.0, 100.0]] * 3)]
    frames = [(40, 21), (90, 122)]

    def batch():
        targets = []
        for b, bx, (w1, h1) in zip(bitmaps, boxes, frames):
            t = BoxList(bx, (w1, h1))
            t.add_field("masks", _rle_masks(b).resize((w1, h1)).transpose(0))
            targets.append(t.to(DEV))
        return targets

    def run(targets):
        transform.decode_masks(targets)
        return [_C.project_rle_masks(t.get_field("masks"), torch.arange(len(t), device=DEV), t.bbox, 14) for t in targets]

    run(batch())   # code objects loaded, allocator warm
    transform.flush()
    targets = batch()
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    honoured = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
        except RuntimeError:
            honoured = True
        got = run(targets) if honoured else None
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert honoured, "torch.cuda.set_sync_debug_mode('error') did not make .item() raise: the check below would show nothing"
    transform.flush()
    assert targets[0].get_field("masks").words is targets[1].get_field("masks").words   # one decode call, one word buffer
    for g, b, bx, (w1, h1) in zip(got, bitmaps, boxes, frames):
        assert np.array_equal(g.cpu().numpy(), rt.project(b, np.arange(len(bx)), bx.numpy(), (h1, w1), True, False, 14))


# ---- one training step from an RLE annotation file ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    paths = tiny_coco.write(tmp_path_factory.mktemp("tiny_rle_coco"))
    paths["instances_bitmap"] = tiny_rle_coco.write(paths)
    return paths


@pytest.fixture(scope="module")
def cfg():
    return tiny_coco.small_cfg()


def _dataset(cfg, paths, ann_file):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCOCapDetDataset

    return COCOCapDetDataset(ann_file, paths["captions"], paths["img_dir"], True, extra_args=cfg.DATASETS.DATASET_ARGS,
                             vocab_file=paths["vocab"])


def _expected_targets(dataset, index, target, boxes, M):
    """The restatement's targets for ``boxes`` matched to the instances of ``target`` in order (proposal p = instance p)."""
    image_id = dataset.ids[index]
    ann_ids = [a["id"] for a in dataset.coco.anns(image_id) if a["iscrowd"] == 0]
    bitmaps = np.stack([tiny_rle_coco.bitmaps()[a] for a in ann_ids])
    m = target.get_field("masks")
    assert m.ann_ids == ann_ids and m.image_id == image_id and m.source_hw == bitmaps.shape[1:]
    return rt.project(bitmaps[m.instance.cpu().numpy()], np.arange(len(boxes)), boxes.cpu().numpy(), (m.size[1], m.size[0]),
                      m.flip_h, m.flip_v, M)


def test_one_training_step_from_an_rle_file(cfg, paths):
    """Loader workers -> prefetcher -> device transform (one decode call per batch) -> the mask loss' targets, which must be
    the restatement's for the bitmaps the file was written from, and a finite step of the tiny student-teacher model."""
    from tests.tiny_model import build_tiny
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import comm, solver, trainer
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import MaskRCNNLossComputation
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList, RleMasks

    dataset = _dataset(cfg, paths, paths["instances_bitmap"])
    transform = build_transforms(cfg, is_train=True)
    loader = make_data_loader(cfg, dataset, transform, True, 0, 1, num_workers=2, seed=4, max_iter=3)
    reports = []

    def spy(batch):
        reports.append(batch[0]["loader"]["indices"])
        return transform(batch)

    stream = DevicePrefetcher(loader, DEV, depth=2, transform=spy)
    try:
        batches = list(stream)
    finally:
        stream.close()
    assert len(batches) == 3
    loss_fn = MaskRCNNLossComputation(cfg)
    M, seen = cfg.MODEL.ROI_MASK_HEAD.RESOLUTION, 0
    for (images, targets), indices in zip(batches, reports):
        proposals = []
        for t in targets:
            p = BoxList(t.bbox.clone(), t.size)   # every ground-truth box as its own proposal: IoU 1 with its instance
            proposals.append(p)
        labels, masks = loss_fn.prepare_targets(proposals, targets)
        for t, index, lab, got in zip(targets, indices, labels, masks):
            m = t.get_field("masks")
            if not isinstance(m, RleMasks):
                continue   # image 101 keeps its polygons
            assert m.words is not None and m.words.is_cuda and len(m) == len(t) and m.size == t.size
            assert torch.equal(lab, t.get_field("labels"))
            want = _expected_targets(dataset, index, t, t.bbox, M)
            assert np.array_equal(got.cpu().numpy(), want), (dataset.ids[index], int((got.cpu().numpy() != want).sum()))
            assert want.any()
            seen += 1
    assert seen >= 2   # of images 7, 12, 55 and 90

    images, targets = batches[0]
    model, e_vocab, _, _, _ = build_tiny("student_teacher_mask_rcnn_uncertainty")
    net = copy.deepcopy(model).cuda()
    net.set_class_embeddings(dataset.class_emb_mtx.cuda())
    net.set_caption_vocab(e_vocab.cuda())
    net.train()
    opt = solver.make_optimizer(cfg, net)
    red = comm.BucketedGradReducer(net)
    torch.manual_seed(100)
    losses = {k: float(v.detach()) for k, v in trainer.train_step(net, opt, red, images, targets).items()}
    red.remove()
    print("losses on the RLE batch:", losses)
    assert "loss_mask" in losses and all(v == v and abs(v) < 1e6 for v in losses.values()), losses


def test_a_malformed_encoding_raises_by_the_next_batch(cfg, paths):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms

    def truncate(data):   # annotation 3 (image 7, compressed): its last character is lost
        for a in data["annotations"]:
            if a["id"] == 3:
                a["segmentation"] = dict(a["segmentation"], counts=a["segmentation"]["counts"][:-1])

    dataset = _dataset(cfg, paths, tiny_rle_coco.write(paths, "instances_malformed", truncate))
    transform = build_transforms(cfg, is_train=True)
    loader = make_data_loader(cfg, dataset, transform, True, 0, 1, num_workers=0, seed=4, max_iter=6)   # two passes over the data
    transformed = []

    def spy(batch):
        transformed.append(batch[0]["loader"]["indices"])
        return transform(batch)

    stream = DevicePrefetcher(loader, DEV, depth=2, transform=spy)
    handed_out = 0
    with pytest.raises(ValueError, match=r"image 7: annotation 3: malformed RLE segmentation: ") as err:
        try:
            for _ in stream:
                handed_out += 1
        finally:
            stream.close()
    bad = next(k for k, idx in enumerate(transformed) if 0 in idx)   # image 7 is dataset index 0
    assert handed_out == bad + 1    # the batch itself came through; the next transform (or the end of the iterator) raised
    assert len(transformed) <= bad + 2
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    assert any(text in str(err.value) for text in _C.COCO_RLE_STATUS.values())
