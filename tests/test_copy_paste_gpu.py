"""GPU: the copy-paste kernels (csrc/copy_paste.hip) and the device half of the input transform against the NumPy restatement
(tests/copy_paste_reference.py).  Everything is compared exactly -- integers and copied float bits -- at the smallest shapes
at which the kernels can go wrong: planes of 1 to 2313 bytes whose starts are not 16-byte aligned, more own masks than a wave
has lanes, canvases that take the 16-byte and the scalar pixel route, in-place swaps and cycles."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import copy_paste_reference as ref
from tests import input_transform_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


# ---- 1. the masks kernel ------------------------------------------------------------------------------------------------------
def _masks_case(h, w, g_own, g_paste, seed):
    """uint8 [g_own + g_paste, h, w], own first: random masks with the special ones the rule cares about."""
    rs = np.random.RandomState(seed)
    own = (rs.rand(g_own, h, w) < 0.4).astype(np.uint8)
    paste = (rs.rand(g_paste, h, w) < 0.25).astype(np.uint8)
    paste[-1, h - 1, w - 1] = 1               # the last byte of the buffer
    paste[0, 0, 0] = 1
    alpha = paste.max(axis=0)
    if g_own >= 1:
        own[0, 0, :] = own[0, h - 1, :] = 1   # set pixels on all four borders
        own[0, :, 0] = own[0, :, w - 1] = 1
    if g_own >= 3:
        own[1] = alpha                        # equal to alpha: nothing is left
        own[2] = 1 - alpha                    # disjoint from it: untouched
    if g_own >= 4:
        own[3] = 0                            # empty before
    return np.concatenate([own, paste])


def _run_masks_raw(masks, num_own, shift):
    """The C entry on buffers of the test's own: masks at byte ``shift`` of one allocation, alpha at an odd offset of another,
    canaries around all of them.  -> (masks after, alpha, table, the bytes that must still be canaries)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _lib

    lib = _lib.load()
    g, h, w = masks.shape
    n = g * h * w
    buf = torch.full((shift + n + 64,), CANARY, dtype=torch.uint8, device="cuda")
    buf[shift:shift + n] = torch.from_numpy(masks.reshape(-1)).cuda()
    a_shift = 16 + (shift * 7) % 16
    abuf = torch.full((a_shift + h * w + 64,), CANARY, dtype=torch.uint8, device="cuda")
    table = torch.full((num_own + 4, 6), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = lib.ovis_copy_paste_masks_u8(buf.data_ptr() + shift, num_own, g - num_own, h, w, abuf.data_ptr() + a_shift,
                                      table.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    buf, abuf, table = buf.cpu().numpy(), abuf.cpu().numpy(), table.cpu().numpy()
    canaries = np.concatenate([buf[:shift], buf[shift + n:], abuf[:a_shift], abuf[a_shift + h * w:]])
    assert (table[num_own:] == 0x5A5A5A5A).all()
    return buf[shift:shift + n].reshape(g, h, w), abuf[a_shift:a_shift + h * w].reshape(h, w), table[:num_own], canaries


@pytest.mark.parametrize("g_own,g_paste", [(0, 1), (1, 1), (3, 2), (70, 3)])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 7), (2, 65), (5, 130), (9, 257)])
def test_masks_kernel_equals_the_reference(h, w, g_own, g_paste):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    masks = _masks_case(h, w, g_own, g_paste, seed=h * 1000 + w + g_own)
    want_alpha = ref.alpha_of(masks[g_own:], (h, w))
    want_own, want_table = ref.cover(masks[:g_own], want_alpha)
    for shift in (0, 5):
        got, alpha, table, canaries = _run_masks_raw(masks, g_own, shift)
        assert (canaries == CANARY).all(), "a byte outside the masks or alpha was written"
        assert np.array_equal(alpha, want_alpha)
        assert np.array_equal(table, want_table)
        assert np.array_equal(got[:g_own], want_own) and np.array_equal(got[g_own:], masks[g_own:])
        again = _run_masks_raw(masks, g_own, shift)
        assert np.array_equal(again[2], table) and np.array_equal(again[0], got)  # the same words on every call
    if g_own >= 3:  # the special masks: equal to alpha, disjoint from it, empty before
        assert want_table[1, 0] > 0 and want_table[1, 1] == 0 and want_table[2, 0] == want_table[2, 1]
    if g_own >= 4:
        assert want_table[3, 0] == 0
    # the shim: the same three results
    dev = torch.from_numpy(masks).cuda()
    alpha, table = _C.copy_paste_masks(dev, g_own)
    assert alpha.dtype == torch.uint8 and table.dtype == torch.int32 and tuple(table.shape) == (g_own, 6)
    assert np.array_equal(alpha.cpu().numpy(), want_alpha) and np.array_equal(table.cpu().numpy(), want_table)
    assert np.array_equal(dev[:g_own].cpu().numpy(), want_own)


def test_masks_kernel_without_pasted_masks_and_bad_arguments():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C, _lib

    masks = _masks_case(3, 7, 2, 1, seed=1)[:2]
    dev = torch.from_numpy(masks).cuda()
    alpha, table = _C.copy_paste_masks(dev, 2)  # num_paste == 0: alpha is written, all zero; nothing is touched
    assert not alpha.any() and np.array_equal(dev.cpu().numpy(), masks)
    assert np.array_equal(table.cpu().numpy(), ref.cover(masks, np.zeros((3, 7), np.uint8))[1])
    lib = _lib.load()
    for args in ((dev.data_ptr(), -1, 1, 3, 7, alpha.data_ptr(), table.data_ptr()), (dev.data_ptr(), 1, 1, 0, 7, alpha.data_ptr(), table.data_ptr()),
                 (dev.data_ptr(), 1, 1, 3, 7, 0, table.data_ptr()), (dev.data_ptr(), 1, 1, 3, 7, alpha.data_ptr(), 0),
                 (0, 1, 1, 3, 7, alpha.data_ptr(), table.data_ptr())):
        assert lib.ovis_copy_paste_masks_u8(*args, 0) == _lib.OVIS_EINVAL
    assert lib.ovis_copy_paste_masks_u8(dev.data_ptr(), 1, 1, 1 << 16, 1 << 15, alpha.data_ptr(), table.data_ptr(), 0) == _lib.OVIS_ERANGE
    with pytest.raises(RuntimeError, match="num_own"):
        _C.copy_paste_masks(dev, 3)


# ---- 2. the images kernel -----------------------------------------------------------------------------------------------------
SPECIAL = [0x7FC00000, 0x7F800001, 0xFFC12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001]  # NaNs, -0.0, infinities, denormals


def _payload(b, c, h, w, seed):
    rs = np.random.RandomState(seed)
    words = rs.randint(0, 2 ** 32, size=(b, c, h, w), dtype=np.uint64).astype(np.uint32)
    flat = words.reshape(-1)
    flat[rs.choice(flat.size, size=min(flat.size, 8 * len(SPECIAL)), replace=False)] = np.array(SPECIAL * 8, dtype=np.uint32)[:min(flat.size, 8 * len(SPECIAL))]
    return words


@pytest.mark.parametrize("pad_h,pad_w", [(8, 12), (5, 67)])
@pytest.mark.parametrize("paste_src", [[1, 0], [1, 2, 0], [2, -1, 0]])
def test_images_kernel_in_place(pad_h, pad_w, paste_src):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    b = len(paste_src)
    words = _payload(b, 3, pad_h, pad_w, seed=pad_w + b)
    rs = np.random.RandomState(7)
    frames = [(pad_h, pad_w), (pad_h - 2, pad_w - 3), (pad_h - 1, pad_w)][:b]  # alpha frames no larger than the canvas
    alphas = [(rs.rand(*f) < 0.5).astype(np.uint8) for f in frames]
    alphas[1][:] = 0 if b == 3 and paste_src[1] >= 0 else alphas[1]  # one alpha all zero (the cycle)
    for a in alphas[:1]:
        a[0, 0] = a[-1, -1] = a[0, -1] = a[-1, 0] = 1
    want = ref.paste_pixels(words, alphas, paste_src)
    assert not np.array_equal(want, words)
    batch = torch.from_numpy(words.view(np.int32)).cuda().view(torch.float32)
    dev_alphas = [torch.from_numpy(a).cuda() if s >= 0 else None for a, s in zip(alphas, paste_src)]
    out = _C.copy_paste_images(batch, dev_alphas, paste_src)
    assert out is batch
    assert np.array_equal(batch.view(torch.int32).cpu().numpy().view(np.uint32), want)


def test_images_kernel_batch_bound_and_bad_arguments():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    n = _C.COPY_PASTE_MAX_IMAGES
    assert n == 16
    words = _payload(n + 1, 1, 4, 8, seed=3)
    alpha = torch.ones((4, 8), dtype=torch.uint8, device="cuda")
    # the largest batch the entry takes: a cycle over all of it
    batch = torch.from_numpy(words[:n].view(np.int32)).cuda().view(torch.float32)
    cycle = [(i + 1) % n for i in range(n)]
    _C.copy_paste_images(batch, [alpha] * n, cycle)
    assert np.array_equal(batch.view(torch.int32).cpu().numpy().view(np.uint32), ref.paste_pixels(words[:n], [np.ones((4, 8), np.uint8)] * n, cycle))
    # one image more: the error, and nothing is written
    batch = torch.from_numpy(words.view(np.int32)).cuda().view(torch.float32)
    with pytest.raises(RuntimeError, match="OVIS_ERANGE"):
        _C.copy_paste_images(batch, [alpha] * (n + 1), [(i + 1) % (n + 1) for i in range(n + 1)])
    torch.cuda.synchronize()
    assert np.array_equal(batch.view(torch.int32).cpu().numpy().view(np.uint32), words)
    small = batch[:2].contiguous()
    for alphas, src in (([alpha, alpha], [2, 0]), ([alpha, alpha], [-2, 0]), ([torch.ones((5, 8), dtype=torch.uint8, device="cuda"), alpha], [1, 0])):
        with pytest.raises(RuntimeError, match="OVIS_EINVAL"):
            _C.copy_paste_images(small, alphas, src)
    with pytest.raises(RuntimeError, match="alpha"):
        _C.copy_paste_images(small, [None, alpha], [1, 0])
    assert np.array_equal(small.view(torch.int32).cpu().numpy().view(np.uint32), words[:2])


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------
SEED = 7  # chosen on the CPU (the search is the three assertions of the test, over seeds 0..): both images paste, one own
#            instance is dropped and one is clipped


def _rect(x1, y1, x2, y2):
    return [[x1, y1, x2, y1, x2, y2, x1, y2]]


def _e2e_inputs():
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList, PolygonMasks

    def target(h, w, rects, labels):
        t = BoxList(torch.tensor(rects, dtype=torch.float32), (w, h))
        t.add_field("labels", torch.tensor(labels, dtype=torch.int64))
        t.add_field("masks", PolygonMasks([_rect(*r) for r in rects], (w, h)))
        return t

    images = [np.random.RandomState(k).randint(0, 256, s + (3,)).astype(np.uint8) for k, s in enumerate(((40, 56), (48, 32)))]
    targets = [target(40, 56, [[4, 4, 50, 36], [10, 10, 20, 20], [30, 2, 52, 12], [2, 28, 12, 38]], [1, 2, 3, 4]),
               target(48, 32, [[2, 2, 28, 40], [6, 8, 16, 18], [18, 30, 30, 46], [1, 20, 9, 30]], [5, 6, 7, 8])]
    return images, targets


def _transforms(seed):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import InputTransform

    make = lambda cp: InputTransform((96,), 160, 0.5, 0.0, T.MEAN, T.STD_COCO, True, seed=seed, scale_jitter=(0.6, 1.2),  # noqa: E731
                                     crop_size=(64, 64), copy_paste=cp)
    return make(None), make(1.0)


def _expected(seed):
    """The reference's composition from the PRE-paste host half (the same per-image draws) on the CPU: per image (alpha,
    boxes, labels, dense masks) or None, the frames, and the facts the seed was chosen for."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _cpu

    images, targets = _e2e_inputs()
    plain, pasting = _transforms(seed)
    base_raw, base = plain.host(images, targets)
    raw, out = pasting.host(images, targets)
    src = raw["paste_src"].tolist()
    want, facts = [], {"pasted": 0, "dropped": 0, "clipped": 0}
    for i, j in enumerate(src):
        if j < 0:
            want.append(None)
            continue
        h, w = raw["image_sizes"][i]
        holder = out[i].get_field("masks")
        n_own = holder.num_own
        picked_boxes, picked_labels = out[i].bbox[n_own:].numpy(), out[i].get_field("labels")[n_own:].numpy()

        def raster(p):
            p = p._with(size=(w, h))
            return _cpu.polygons_to_masks(p.coords, p.polygon_start, p.instance_start, p.size).numpy()

        own = raster(base[i].get_field("masks"))
        both = raster(holder.polygons)
        assert np.array_equal(both[:n_own], own)
        res = ref.paste_image_targets(own, base[i].bbox.numpy(), base[i].get_field("labels").numpy(), both[n_own:], picked_boxes,
                                      picked_labels, (h, w))
        _, table = ref.cover(own, res[0])
        keep, _ = ref.keep_rule(table, base[i].bbox.numpy())
        facts["pasted"] += 1
        facts["dropped"] += n_own - len(keep)
        facts["clipped"] += sum(1 for g in keep if table[g][0] != table[g][1])
        want.append(res)
    return (images, targets), base_raw, (raw, out), want, facts


def test_end_to_end_equals_the_reference_composition():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import project_gt_masks, project_masks_on_boxes

    _, base_raw, (raw, out), want, facts = _expected(SEED)
    assert facts["pasted"] == 2 and facts["dropped"] >= 1 and facts["clipped"] >= 1, facts  # not vacuous
    pasting = _transforms(SEED)[1]
    staged = DevicePrefetcher([(raw, out)], "cuda", transform=pasting)
    try:
        images, targets = next(iter(staged))
    finally:
        staged.close()
    torch.cuda.synchronize()
    # pixels: transform_images_window's own output, composed by the reference
    plain = _C.transform_images_window(base_raw["data"].cuda(), base_raw["desc"].cuda(), T.MEAN, T.STD_COCO, True, base_raw["pad_hw"],
                                       base_raw["max_in_hw"])
    words = plain.view(torch.int32).cpu().numpy().view(np.uint32)
    composed = ref.paste_pixels(words, [w[0] if w is not None else None for w in want], raw["paste_src"].tolist())
    assert not np.array_equal(composed, words)
    assert np.array_equal(images.tensors.view(torch.int32).cpu().numpy().view(np.uint32), composed)
    assert images.image_sizes == [tuple(s) for s in raw["image_sizes"]]
    for t, w, (h_, w_) in zip(targets, want, raw["image_sizes"]):
        _, boxes, labels, dense = w
        assert t.size == (w_, h_)
        assert np.array_equal(t.bbox.cpu().numpy(), boxes) and t.bbox.dtype == torch.float32
        assert np.array_equal(t.get_field("labels").cpu().numpy(), labels)
        got = t.get_field("masks")
        assert torch.is_tensor(got) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), dense)
        index = torch.arange(len(t), device="cuda")
        assert torch.equal(project_gt_masks(got, index, t.bbox, 28), project_masks_on_boxes(got, index, t.bbox, 28))


# ---- 4. training ----------------------------------------------------------------------------------------------------------------
def test_training_with_copy_paste_is_finite_and_reproducible(tmp_path, monkeypatch):
    """Two iterations of the teacher configuration over tests/tiny_coco.py (the raw-input configuration of
    tests/test_train_eval_gpu.py) with --scale-jitter 0.5 1.5 --crop-size 128 128 --copy-paste 1.0, twice from the same seeds:
    finite and equal losses, and pastes did happen.  The 128 x 128 canvas runs as it is."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from tests import tiny_coco

    spec = importlib.util.spec_from_file_location("ovis_tool_train_net", os.path.join(ROOT, "tools", "train_net.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    paths = tiny_coco.write(tmp_path)
    pasted = []
    real = _C.copy_paste_images
    monkeypatch.setattr(_C, "copy_paste_images", lambda batch, alphas, src: (pasted.append(list(src)), real(batch, alphas, src))[1])
    histories = []
    for _ in range(2):
        cfg = tiny_coco.small_cfg("zeroshot_mask", extra=["DATALOADER.NUM_WORKERS", 0, "SOLVER.LOG_PERIOD", 1, "SOLVER.BASE_LR", 0.005,
                                                          "SOLVER.WARMUP_ITERS", 0])
        torch.manual_seed(1234)
        histories.append(tool.train(cfg, 0, False, 2, 2, dataset_catalog=paths["catalog"], data_dir=paths["root"], seed=5,
                                    scale_jitter=(0.5, 1.5), crop_size=(128, 128), copy_paste=1.0))
        torch.cuda.synchronize()
    a, b = histories
    assert len(a) == 2 and a == b, (a, b)
    assert all(math.isfinite(v) for _, vals in a for v in vals.values())
    assert pasted and any(s >= 0 for src in pasted for s in src)
