"""CPU: the colour-jitter arithmetic by exact equality.  tests/golden/color_jitter.npz holds what PIL itself produced
(make_color_jitter_golden.py); tests/color_jitter_reference.py is a NumPy restatement of the rule of include/ovis_hip.h.
The restatement is pinned to the fixture (and to PIL itself where it is installed), the host twin (libovis_cpu.so) to the
restatement; tests/test_color_jitter_gpu.py pins the device kernels to both."""
import os
import zlib

import numpy as np
import pytest
import torch

from tests import color_jitter_reference as R
from tests.golden import make_color_jitter_golden as G

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_jitter.npz"))
SMALL = {"half": G.half_mean_image, "constant": G.constant_image, "pixel": G.one_pixel}
CONTRAST_ONLY = [([1, -1, -1, -1], [f, 0.0, 0.0, 0.0]) for f in (0.0, 2.0)]


def _twin(img, ops, params):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    data, desc = R.pack([img])
    out = _C.color_jitter(torch.from_numpy(data), torch.from_numpy(desc), torch.tensor([ops], dtype=torch.int32),
                          torch.tensor([params], dtype=torch.float32))
    assert not out.is_cuda and out.dtype == torch.uint8
    return out.numpy().reshape(img.shape)


@pytest.fixture(scope="module")
def hue_of_all_colours():
    """The restatement's hue at the five shifts over all 2^24 colours, computed once."""
    return dict(zip(G.SHIFTS, R.hue_many(R.all_colours(), G.SHIFTS)))


def test_fixture_inputs_did_not_drift():
    assert np.array_equal(GOLD["img"], G.seeded_image())
    assert str(GOLD["pil_version"]).split(".")[0].isdigit()


def test_hue_over_all_colours_equals_the_fixture_pil_and_the_host_twin(hue_of_all_colours):
    colours = R.all_colours()
    for k, shift in enumerate(G.SHIFTS):
        want = hue_of_all_colours[shift]
        assert zlib.crc32(want.tobytes()) == int(GOLD["hue_crc"][k]), f"shift {shift}"
        assert np.array_equal(_twin(colours, [3, -1, -1, -1], [float(shift), 0.0, 0.0, 0.0]), want), f"shift {shift}"
    assert not np.array_equal(hue_of_all_colours[0], colours)   # the round trip is not the identity
    assert np.array_equal(R.hue(colours[:48], 127), hue_of_all_colours[127][:48])   # the table form == the direct form


def test_hue_over_all_colours_equals_installed_pil(hue_of_all_colours):
    pytest.importorskip("PIL.Image")
    colours = R.all_colours()
    for shift in G.SHIFTS:
        assert np.array_equal(G.pil_chain(colours, [3, -1, -1, -1], [float(shift), 0, 0, 0]), hue_of_all_colours[shift]), shift


def test_blend_over_every_pair_equals_the_fixture_and_the_host_twin():
    d, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    assert G.FACTORS[3] == float(np.float32(1) + np.float32(2.0 ** -23)) and 0 < G.FACTORS[1] < 1
    # The twin has no blend entry of its own: contrast it is.  Image d of a batch of 256 is 257 x 256: one row holding every
    # grey x once, 256 rows of grey d -- its mean is d + (32640 - 256 d) / 65792, less than half a level from d, so the
    # degenerate value is d and the first row comes out as blend(d, x, f).
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    images = np.empty((256, 257, 256, 3), dtype=np.uint8)
    images[:] = np.arange(256, dtype=np.uint8)[:, None, None, None]
    images[:, 0] = np.arange(256, dtype=np.uint8)[None, :, None]
    assert [R.contrast_mean(images[k]) for k in (0, 1, 127, 128, 255)] == [0, 1, 127, 128, 255]
    data, desc = R.pack(list(images))
    data, desc, ops = torch.from_numpy(data), torch.from_numpy(desc), torch.tensor([[1, -1, -1, -1]] * 256, dtype=torch.int32)
    for k, f in enumerate(G.FACTORS):
        got = R.blend(d, x, f)
        assert np.array_equal(got, GOLD["blend"][k]), f
        out = _C.color_jitter(data, desc, ops, torch.tensor([[f, 0.0, 0.0, 0.0]] * 256)).numpy().reshape(images.shape)
        assert np.array_equal(out[:, 0, :, 0], got) and np.array_equal(out[:, 0, :, 2], got), f
        assert np.array_equal(out[:, 1:], images[:, 1:]), f   # blend(d, d, f) == d for every factor


def test_blend_equals_installed_pil():
    pytest.importorskip("PIL.Image")
    for k, f in enumerate(G.FACTORS):
        assert np.array_equal(G.pil_blend_table(f), GOLD["blend"][k]), f


def test_grey_is_pils_l_conversion():
    Image = pytest.importorskip("PIL.Image")
    img = np.random.RandomState(3).randint(0, 256, (64, 64, 3)).astype(np.uint8)
    assert np.array_equal(R.grey(img), np.asarray(Image.fromarray(img).convert("L")))


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_images_equal_the_fixture_and_the_host_twin(name):
    """A contrast mean of exactly 10.5, a constant image and a 1 x 1 image: all 24 orders, then contrast at 0 and 2."""
    img = SMALL[name]()
    rows = [G.row(o) for o in G.ORDERS] + CONTRAST_ONLY
    for k, (ops, params) in enumerate(rows):
        want = R.apply_chain(img, ops, params)
        assert np.array_equal(want, GOLD[name][k]), (name, ops)
        assert np.array_equal(_twin(img, ops, params), want), (name, ops)
    if name == "half":
        assert R.contrast_mean(img) == 11 and GOLD["half"][24].reshape(-1).tolist() == [11] * 6


def test_every_order_and_every_subset_equal_the_fixture_and_the_host_twin():
    img = GOLD["img"]
    for key, chains in (("orders", G.ORDERS), ("subsets", G.SUBSETS)):
        assert len(chains) == len(GOLD[key])
        for k, chain in enumerate(chains):
            ops, params = G.row(chain)
            want = R.apply_chain(img, ops, params)
            assert np.array_equal(want, GOLD[key][k]), (key, chain)
            assert np.array_equal(_twin(img, ops, params), want), (key, chain)
    assert np.array_equal(GOLD["subsets"][0], img)   # the empty chain
    for k, shift in enumerate(G.SHIFTS):
        assert np.array_equal(R.hue(img, shift), GOLD["hue_small"][k])


def test_every_order_and_every_subset_equal_installed_pil():
    pytest.importorskip("PIL.Image")
    img = G.seeded_image(19, 31, seed=5)
    rng = np.random.RandomState(0)
    for chain in G.ORDERS + G.SUBSETS:
        ops, _ = G.row(chain)
        params = [float(np.float32(rng.uniform(0.2, 1.9))) if o in (0, 1, 2) else float(rng.randint(0, 256)) if o == 3 else 0.0
                  for o in ops]
        assert np.array_equal(G.pil_chain(img, ops, params), R.apply_chain(img, ops, params)), (ops, params)


def test_malformed_rows_copy_and_bad_arguments_raise():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    img = GOLD["img"]
    for ops in ([4, -1, -1, -1], [-2, -1, -1, -1], [0, 0, -1, -1], [-1, 0, -1, -1], [0, -1, 1, -1], [1, 2, 3, 1]):
        assert np.array_equal(_twin(img, ops, [1.3, 0.6, 1.7, 37.0]), img), ops
        assert np.array_equal(R.apply_chain(img, ops, [1.3, 0.6, 1.7, 37.0]), img), ops
    # a hue parameter that is no shift 0..255 shifts by 0; a factor that is not finite stays inside 0..255
    assert np.array_equal(_twin(img, [3, -1, -1, -1], [300.0, 0, 0, 0]), R.hue(img, 0))
    for f in (float("inf"), float("nan"), -3.0, 1e30):
        assert np.array_equal(_twin(img, [0, -1, -1, -1], [f, 0, 0, 0]), R.brightness(img, f)), f
    data, desc = R.pack([img])
    data, ops, params = torch.from_numpy(data), torch.tensor([[0, -1, -1, -1]], dtype=torch.int32), torch.ones(1, 4)
    for bad in ([1, 16, 23], [0, 17, 23], [-3, 16, 23], [0, 0, 23]):
        with pytest.raises(RuntimeError, match="color_jitter"):
            _C.color_jitter(data, torch.tensor([bad + [1, 1, 0, 0]], dtype=torch.int32), ops, params)
    with pytest.raises(RuntimeError, match="color_jitter"):
        _C.color_jitter(data, torch.from_numpy(desc), ops[:, :3], params)
    empty = _C.color_jitter(data[:0], torch.zeros(0, 7, dtype=torch.int32), ops[:0], params[:0])
    assert empty.numel() == 0
