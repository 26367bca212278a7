"""GPU: the device colour jitter (csrc/color_jitter.hip) == its host twin == the NumPy restatement
(tests/color_jitter_reference.py), byte for byte; the restatement and the twin are pinned to PIL in
tests/test_color_jitter_reference.py.  The apply kernel gives a block 1024 pixels and a thread 4; the sum kernel strides
256 blocks over an image, one round = 262144 pixels."""
import os
import random

import numpy as np
import pytest
import torch

from tests import color_jitter_reference as R
from tests.golden import make_color_jitter_golden as G

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_jitter.npz"))
BLOCK_PIXELS, THREAD_PIXELS, SUM_ROUND_PIXELS = 1024, 4, 256 * 1024
ALL_FOUR = ([0, 1, 2, 3], [1.3, 0.6, 1.7, 37.0])


def _image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _three_ways(images, rows, contrast=True):
    """-> (device bytes, host-twin bytes, restatement bytes) of a batch; rows = [(ops, params)] per image."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    data, desc = R.pack(images)
    ops = np.array([r[0] for r in rows], dtype=np.int32)
    params = np.array([r[1] for r in rows], dtype=np.float32)
    t = [torch.from_numpy(a) for a in (data, desc, ops, params)]
    max_in = (max(i.shape[0] for i in images), max(i.shape[1] for i in images))
    got = _C.color_jitter(*[a.cuda() for a in t], max_in, contrast=contrast)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == t[0].shape
    return got.cpu().numpy(), _C.color_jitter(*t).numpy(), R.apply_batch(data, desc, ops, params)


def _assert_equal(images, rows, **kw):
    got, twin, want = _three_ways(images, rows, **kw)
    assert np.array_equal(twin, want), "host twin != restatement"
    assert np.array_equal(got, want), f"device != restatement at bytes {np.flatnonzero(got != want)[:8]}"
    return got


def test_mixed_batch_contrast_first_middle_last():
    images = [_image(33, 41, s) for s in range(5)]
    rows = [([-1] * 4, [0.0] * 4), ALL_FOUR, ([1, 0, 3, -1], [0.6, 1.3, 200.0, 0.0]), ([2, 1, 0, -1], [0.2, 1.9, 0.7, 0.0]),
            ([3, 2, 0, 1], [128.0, 1.7, 1.1, 0.5])]
    got = _assert_equal(images, rows)
    assert np.array_equal(got[:3 * 33 * 41], images[0].reshape(-1))   # no operation: a copy
    assert np.array_equal(got, _three_ways(images, rows)[0]), "two runs differ"


def test_offsets_of_every_residue_and_the_smallest_images():
    images = [_image(5, 7, 1), _image(3, 3, 2), _image(1, 1, 3), _image(3, 3, 4), _image(1, 1, 5)]
    _, desc = R.pack(images)
    assert {int(o) % 4 for o in desc[:, 0]} == {0, 1, 2, 3}
    _assert_equal(images, [ALL_FOUR, ([3, 1, -1, -1], [5.0, 1.5, 0.0, 0.0]), ALL_FOUR, ([1, -1, -1, -1], [0.5, 0, 0, 0]),
                           ([2, 3, 1, 0], [1.7, 37.0, 0.6, 1.3])])


@pytest.mark.parametrize("pixels", [THREAD_PIXELS - 1, THREAD_PIXELS, THREAD_PIXELS + 1, BLOCK_PIXELS - 1, BLOCK_PIXELS,
                                    BLOCK_PIXELS + 1])
def test_pixel_counts_around_a_thread_and_a_block(pixels):
    # a one-pixel image in front makes the offset odd
    _assert_equal([_image(1, 1, 0), _image(1, pixels, pixels)], [ALL_FOUR, ([0, 3, 1, 2], [0.8, 250.0, 1.4, 0.3])])


def test_image_larger_than_one_round_of_the_sum_kernel():
    img = _image(513, 512, 11)
    assert img.shape[0] * img.shape[1] > SUM_ROUND_PIXELS
    _assert_equal([img, _image(2, 3, 12)], [([0, 1, -1, -1], [1.2, 1.6, 0.0, 0.0]), ALL_FOUR])


def test_contrast_means():
    half, black = G.half_mean_image(), np.zeros((6, 5, 3), dtype=np.uint8)
    for f in (0.0, 2.0, 0.5):
        rows = [([1, -1, -1, -1], [f, 0.0, 0.0, 0.0])] * 2
        got = _assert_equal([half, black], rows)
        if f == 0.0:
            assert got[:6].tolist() == [11] * 6   # the mean 10.5 rounds to 11
        assert not got[6:].any()
    # contrast in the table but contrast=False (no workspace): those images are copied, the others jittered
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    img = _image(9, 11, 3)
    data, desc = R.pack([img, img])
    ops = np.array([[1, -1, -1, -1], [0, -1, -1, -1]], dtype=np.int32)
    params = np.array([[1.5, 0, 0, 0], [1.5, 0, 0, 0]], dtype=np.float32)
    got = _C.color_jitter(*[torch.from_numpy(a).cuda() for a in (data, desc, ops, params)], (9, 11), contrast=False).cpu().numpy()
    assert np.array_equal(got[:297], img.reshape(-1)) and np.array_equal(got[297:], R.brightness(img, 1.5).reshape(-1))


def test_hue_shifts_and_the_round_trip_that_is_not_the_identity():
    img = GOLD["img"]
    for k, shift in enumerate(G.SHIFTS):
        got = _assert_equal([img], [([3, -1, -1, -1], [float(shift), 0.0, 0.0, 0.0])])
        assert np.array_equal(got.reshape(img.shape), GOLD["hue_small"][k]), f"shift {shift}: not PIL's bytes"
    assert not np.array_equal(GOLD["hue_small"][0], img)


def test_all_colours_through_hue_equal_the_host_twin():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    data, desc = R.pack([R.all_colours()])
    t = [torch.from_numpy(a) for a in (data, desc, np.array([[3, -1, -1, -1]], dtype=np.int32),
                                       np.array([[127, 0, 0, 0]], dtype=np.float32))]
    got = _C.color_jitter(*[a.cuda() for a in t], (4096, 4096), contrast=False)
    assert torch.equal(got.cpu(), _C.color_jitter(*t))


@pytest.mark.parametrize("guard", [64, 61])   # 61: out has another misalignment than data -- the byte-wise loads
def test_invalid_descriptors_and_malformed_rows_touch_nothing_else(guard):
    """The raw entry point with guard bytes around out and the workspace."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    img = _image(30, 40, 21)
    n = img.size
    data = torch.from_numpy(np.concatenate([img.reshape(-1), img.reshape(-1)])).cuda()
    good = [0, 30, 40, 30, 40, 0, 0]
    bad_descs = ([n, 31, 40, 31, 40, 0, 0], [n + 3, 30, 40, 30, 40, 0, 0], [-1, 30, 40, 30, 40, 0, 0], [n, 0, 40, 30, 40, 0, 0],
                 [n, 30, 41, 30, 40, 0, 0])
    bad_rows = ([4, -1, -1, -1], [-2, -1, -1, -1], [0, 0, -1, -1], [-1, 0, -1, -1], [0, -1, 1, -1], [1, 2, 3, 1])
    want_good = R.apply_chain(img, *ALL_FOUR).reshape(-1)

    def run(desc, rows):
        out_full = torch.full((2 * n + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
        ws_full = torch.full((16 + 16 + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        ops = torch.tensor(rows, dtype=torch.int32).cuda()
        params = torch.tensor([ALL_FOUR[1]] * 2, dtype=torch.float32).cuda()
        rc = _C._L.ovis_color_jitter_u8(data.data_ptr(), data.numel(), torch.tensor(desc, dtype=torch.int32).cuda().data_ptr(),
                                        ops.data_ptr(), params.data_ptr(), 2, 30, 40, ws_full.data_ptr() + 16, 16,
                                        out_full.data_ptr() + guard, _C._stream())
        assert rc == 0
        torch.cuda.synchronize()
        out_full, ws_full = out_full.cpu().numpy(), ws_full.cpu().numpy()
        assert (out_full[:guard] == 0xA5).all() and (out_full[guard + 2 * n:] == 0xA5).all()
        assert (ws_full[:16] == 0x5A).all() and (ws_full[32:] == 0x5A).all()
        return out_full[guard:guard + 2 * n]

    for bad in bad_descs:
        out = run([good, bad], [ALL_FOUR[0]] * 2)
        assert np.array_equal(out[:n], want_good) and (out[n:] == 0xA5).all(), bad
    for bad in bad_rows:
        out = run([good, [n] + good[1:]], [ALL_FOUR[0], bad])
        assert np.array_equal(out[:n], want_good) and np.array_equal(out[n:], img.reshape(-1)), bad
    # out overlapping data, a misaligned or short workspace, an oversize bound
    lib, s = _C._L, _C._stream()
    desc = torch.tensor([good, good], dtype=torch.int32).cuda()
    ops, params = torch.tensor([ALL_FOUR[0]] * 2, dtype=torch.int32).cuda(), torch.tensor([ALL_FOUR[1]] * 2).cuda()
    ws, out = torch.zeros(32, dtype=torch.uint8, device="cuda"), torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
    args = (desc.data_ptr(), ops.data_ptr(), params.data_ptr(), 2, 30, 40)
    assert lib.ovis_color_jitter_u8(data.data_ptr(), 2 * n, *args, ws.data_ptr(), 16, data.data_ptr() + n, s) == _C._lib.OVIS_EINVAL
    assert lib.ovis_color_jitter_u8(data.data_ptr(), 2 * n, *args, ws.data_ptr() + 4, 16, out.data_ptr(), s) == _C._lib.OVIS_EINVAL
    assert lib.ovis_color_jitter_u8(data.data_ptr(), 2 * n, *args, ws.data_ptr(), 8, out.data_ptr(), s) == _C._lib.OVIS_ENOSPC
    assert lib.ovis_color_jitter_u8(data.data_ptr(), 2 * n, *args[:4], 16385, 40, ws.data_ptr(), 16, out.data_ptr(), s) == _C._lib.OVIS_ERANGE
    assert lib.ovis_color_jitter_workspace_bytes(2) == 16 and lib.ovis_color_jitter_workspace_bytes(0) == 0


def test_jittered_input_transform_on_the_device_equals_the_host():
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import make_raw_batch
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import InputTransform
    from tests import input_transform_ref as T

    t = InputTransform((96, 112), 160, 0.5, 0.5, T.MEAN, T.STD_COCO, True, size_divisible=32, color_jitter=(0.4, 0.4, 0.4, 0.1))
    raw, _ = t.host(*make_raw_batch(3, seed=9, sizes=((48, 64), (61, 43), (50, 50)), num_gt=2), rng=random.Random(9))
    assert raw["jitter_ops"].shape == (3, 4) and sorted(raw["jitter_ops"][0].tolist()) == [0, 1, 2, 3]
    want = t.device(raw)
    got = t.device({k: v.cuda() if torch.is_tensor(v) else v for k, v in raw.items()})
    assert got.tensors.is_cuda and got.image_sizes == want.image_sizes
    assert np.array_equal(got.tensors.cpu().numpy().view(np.uint32), want.tensors.numpy().view(np.uint32))
    plain = InputTransform((96, 112), 160, 0.5, 0.5, T.MEAN, T.STD_COCO, True, size_divisible=32).device(
        {k: v for k, v in raw.items() if not k.startswith("jitter_")})
    assert not np.array_equal(plain.tensors.numpy(), want.tensors.numpy())
