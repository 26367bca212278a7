"""GPU: the weight EMA on the device -- the fused SGD + EMA launch and the swap launch of csrc/optim.hip against their
multi-tensor twins, bit for bit; the cached route of ``GroupFusedSGD`` with an EMA attached; and ``ModelEma.applied`` inside a
live training process of the tiny teacher model (tests/tiny_coco.py, the runs of tests/test_train_eval_gpu.py with ``--ema``):
what the model computes inside the context is what a freshly built model computes from the averaged weights, and training
goes on afterwards as if the context had never been entered."""
import copy
import importlib.util
import json
import os

import pytest
import torch

from tests import tiny_coco

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the shapes of tests/test_solver_gpu.py plus the chunk's neighbours: 1, 81, 4095 / 4096 / 4097, a 2-D tensor of many chunks
SHAPES = [(64, 32, 3, 3), (81,), (4097,), (2048, 512), (1,), (7, 5), (256,), (33, 1000), (4095,), (4096,)]
DECAY = 0.999


class Bag(torch.nn.Module):
    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES])
        self.frozen = torch.nn.Parameter(torch.randn(5, generator=g), requires_grad=False)


def _make(native, momentum=0.9, decayed=True, seed=0):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.ema import ModelEma
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.solver import GroupFusedSGD

    model = Bag(seed).cuda()
    groups = []
    for i, p in enumerate(model.w):
        bias = p.dim() == 1
        groups.append({"params": [p], "lr": 0.02 * (2 if bias else 1) * (10 if i == 4 else 1),
                       "weight_decay": 1e-4 if decayed and not bias else 0.0})
    opt = GroupFusedSGD(groups, 0.02, momentum=momentum)
    opt.native = native
    opt.ema = ModelEma(model, DECAY)
    flat = torch.zeros(sum(p.numel() for p in model.w) + 3, device="cuda")
    off = 3  # every gradient view starts at an odd element offset somewhere
    for p in model.w:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    return model, opt, flat


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _assert_equal_state(step, ma, oa, mb, ob):
    for i, (x, y) in enumerate(zip(ma.w, mb.w)):
        assert _same(x, y), (step, i, "p")
        bx, by = oa.state[x].get("momentum_buffer"), ob.state[y].get("momentum_buffer")
        assert (bx is None) == (by is None) and (bx is None or _same(bx, by)), (step, i, "buf")
        assert _same(oa.ema.tensors[f"w.{i}"], ob.ema.tensors[f"w.{i}"]), (step, i, "ema")
    assert oa.ema.num_updates == ob.ema.num_updates == step + 1


# ---- 1. the fused launch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum,decayed", [(0.9, True), (0.0, False)])
def test_fused_sgd_ema_equals_the_foreach_twin_bit_for_bit(momentum, decayed):
    ma, oa, fa = _make(True, momentum, decayed)
    mb, ob, fb = _make(False, momentum, decayed)
    assert str(oa.ema.tensors["w.0"].device) == str(ma.w[0].device) and oa.ema.tensors["w.0"].is_cuda
    start = [p.detach().clone() for p in ma.w]
    g = torch.Generator().manual_seed(5)
    for step in range(7):
        vals = torch.randn(fa.numel(), generator=g).cuda()
        fa.copy_(vals)
        fb.copy_(vals)
        for opt in (oa, ob):
            for grp in opt.param_groups:
                grp["lr"] *= 0.5 if step == 2 else 1.1   # the schedule moves every group's rate
        oa.step()
        ob.step()
        _assert_equal_state(step, ma, oa, mb, ob)
    assert "fast_ema" in oa._native_tables and oa._native_tables["fast_ema"] is not None   # the native route did run
    for i, p in enumerate(ma.w):   # ... and all three moved, each its own way
        e = oa.ema.tensors[f"w.{i}"]
        assert not _same(p, start[i]) and not _same(e, start[i]) and not _same(e, p), i
    assert _same(ma.frozen, Bag().frozen.cuda())


def test_raw_parameters_and_momentum_equal_the_launch_without_ema():
    ma, oa, fa = _make(True)
    mb, ob, fb = _make(True)
    ob.ema = None
    g = torch.Generator().manual_seed(6)
    for step in range(4):
        vals = torch.randn(fa.numel(), generator=g).cuda()
        fa.copy_(vals)
        fb.copy_(vals)
        oa.step()
        ob.step()
        for x, y in zip(ma.w, mb.w):
            assert _same(x, y) and _same(oa.state[x]["momentum_buffer"], ob.state[y]["momentum_buffer"]), (step, tuple(x.shape))
    assert ob._native_tables.get("fast_ema") is None
    # the tables without an EMA are today's 32-byte records, those with one the 40-byte records
    for (_, with_ema, _), (_, without, _) in zip(oa._native_tables["tables"][2], ob._native_tables["tables"][2]):
        assert without.numel() % 32 == 0 and with_ema.numel() * 32 == without.numel() * 40


# ---- 2. the cached route -------------------------------------------------------------------------------------------------------------
def test_cached_route_in_steady_state_and_what_makes_a_step_leave_it():
    ma, oa, fa = _make(True)
    mb, ob, fb = _make(False)
    g = torch.Generator().manual_seed(9)
    taken = []
    cached = oa._step_cached
    oa._step_cached = lambda groups, *w: (taken.append(cached(groups, *w)), taken[-1])[1]
    count = [0]

    def step():
        vals = torch.randn(fa.numel(), generator=g).cuda()
        fa.copy_(vals)
        fb.copy_(vals)
        oa.step()
        ob.step()
        _assert_equal_state(count[0], ma, oa, mb, ob)
        count[0] += 1

    step()
    step()
    step()
    assert taken == [False, True, True]
    saved = copy.deepcopy(oa.ema.state_dict())
    step()
    # the averages replaced behind the cache's back: new tensors holding the older values
    for o in (oa, ob):
        o.ema.load_state_dict(copy.deepcopy(saved))
    count[0] = saved["num_updates"]
    fresh = [oa.ema.tensors[f"w.{i}"] for i in range(len(SHAPES))]
    step()
    assert all(oa.ema.tensors[f"w.{i}"] is e for i, e in enumerate(fresh))   # the loaded tensors are the ones updated
    step()
    assert taken == [False, True, True, True, False, True]
    for m in (ma, mb):   # new storage behind a parameter
        m.w[3].data = m.w[3].data.clone()
    step()
    step()
    assert taken[6:] == [False, True]
    held = []
    for m in (ma, mb):   # a gradient goes missing: neither the parameter nor its average moves
        held.append(m.w[5].grad)
        m.w[5].grad = None
    before = (ma.w[5].detach().clone(), oa.ema.tensors["w.5"].clone())
    step()
    assert _same(ma.w[5], before[0]) and _same(oa.ema.tensors["w.5"], before[1])
    for m, grad in zip((ma, mb), held):
        m.w[5].grad = grad
    step()
    step()
    assert taken[8:] == [False, False, True]
    # detaching the EMA goes back to the 32-byte tables, attaching it again to the 40-byte ones
    ea, eb = oa.ema, ob.ema
    oa.ema = ob.ema = None
    vals = torch.randn(fa.numel(), generator=g).cuda()
    fa.copy_(vals)
    fb.copy_(vals)
    oa.step()
    ob.step()
    assert taken[-1] is False and ea.num_updates == count[0]
    oa.ema, ob.ema = ea, eb
    step()
    step()
    assert taken[-2:] == [False, True]


# ---- 3. the swap launch --------------------------------------------------------------------------------------------------------------
def test_swap_launch_exchanges_every_bit_pattern_and_two_swaps_are_the_identity():
    import numpy as np

    from cvpr22_cross_modal_pseudo_labeling_amd import _C, _lib

    chunk = _C.sgd_chunk_elements()
    sizes = [1, chunk - 1, chunk, chunk + 1, 3 * chunk + 17]
    g = torch.Generator().manual_seed(3)
    # every bit pattern is fair: random words hold NaNs with payloads, infinities, subnormals; the specials are planted too
    special = torch.tensor([0x7FC00001, -0x3FFFFF, 0x7F800001, -0x800000, -0x80000000, 0, 1, -0x7FFFFFFF, 0x007FFFFF, 0x7F800000],
                           dtype=torch.int64)
    a_words, b_words = [], []
    for n in sizes:
        x = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64)
        y = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64)
        k = min(n, len(special))
        x[:k] = special[:k]
        y[n - k:] = special[:k].flip(0)
        a_words.append(x.to(torch.int32).cuda())
        b_words.append(y.to(torch.int32).cuda())
    # every tensor sits at an odd element offset between guard words
    guard = 0x5A5A5A5A

    def guarded(words):
        room = torch.full((words.numel() + 7,), guard, dtype=torch.int32, device="cuda")
        room[3:3 + words.numel()] = words
        return room

    want_a, want_b = [t.clone() for t in a_words], [t.clone() for t in b_words]
    rooms = [guarded(t) for t in a_words + b_words]
    a = [r[3:r.numel() - 4].view(torch.float32) for r in rooms[:len(sizes)]]
    b = [r[3:r.numel() - 4].view(torch.float32) for r in rooms[len(sizes):]]
    items = np.array([(x.data_ptr(), y.data_ptr(), x.numel()) for x, y in zip(a, b)], dtype=np.int64)
    blocks = [(j, c) for j, n in enumerate(sizes) for c in range((n + chunk - 1) // chunk)]
    items_d = torch.from_numpy(items.view(np.uint8).reshape(-1)).cuda()
    blocks_d = torch.tensor(blocks, dtype=torch.int32, device="cuda").reshape(-1, 2)
    _C.swap_multi(items_d, blocks_d)
    for x, y, wa, wb in zip(a, b, want_a, want_b):
        assert torch.equal(x.view(torch.int32), wb) and torch.equal(y.view(torch.int32), wa), x.numel()
    _C.swap_multi(items_d, blocks_d)
    for x, y, wa, wb in zip(a, b, want_a, want_b):
        assert torch.equal(x.view(torch.int32), wa) and torch.equal(y.view(torch.int32), wb), x.numel()
    # the argument checks of the two entries follow ovis_sgd_momentum_multi_f32
    lib = _lib.load()
    assert lib.ovis_swap_multi_f32(items_d.data_ptr(), blocks_d.data_ptr(), -1, None) == _lib.OVIS_EINVAL
    assert lib.ovis_swap_multi_f32(None, None, 0, None) == _lib.OVIS_OK
    assert lib.ovis_swap_multi_f32(None, blocks_d.data_ptr(), 1, None) == _lib.OVIS_EINVAL
    assert lib.ovis_swap_multi_f32(items_d.data_ptr(), None, 1, None) == _lib.OVIS_EINVAL
    assert lib.ovis_sgd_momentum_ema_multi_f32(items_d.data_ptr(), blocks_d.data_ptr(), -1, .1, 0., .9, 0, .1, None) == _lib.OVIS_EINVAL
    assert lib.ovis_sgd_momentum_ema_multi_f32(None, None, 0, .1, 0., .9, 0, .1, None) == _lib.OVIS_OK
    assert lib.ovis_sgd_momentum_ema_multi_f32(None, blocks_d.data_ptr(), 1, .1, 0., .9, 0, .1, None) == _lib.OVIS_EINVAL
    assert lib.ovis_sgd_momentum_ema_multi_f32(items_d.data_ptr(), None, 1, .1, 0., .9, 0, .1, None) == _lib.OVIS_EINVAL
    torch.cuda.synchronize()
    for x, wa in zip(a, want_a):
        assert torch.equal(x.view(torch.int32), wa)
    for r in rooms:
        assert bool((r[:3] == guard).all()) and bool((r[-4:] == guard).all())
    with pytest.raises(RuntimeError, match="HIP device"):
        _C.swap_multi(items_d.cpu(), blocks_d)


def test_applied_on_the_device_swaps_in_one_launch_and_restores_every_bit():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.layers import pair_bottleneck

    model, opt, flat = _make(True)
    flat.copy_(torch.randn(flat.numel(), generator=torch.Generator().manual_seed(1)).cuda())
    opt.step()
    opt.step()
    avg = opt.ema
    model.w[1].data[:4] = torch.tensor([float("nan"), -0.0, 1e-42, float("-inf")], device="cuda")
    raw, mean = [p.detach().clone() for p in model.w], [e.clone() for e in avg.tensors.values()]
    pointers = [(p.data_ptr(), e.data_ptr()) for p, e in zip(model.w, avg.tensors.values())]
    calls = []
    real = _C.swap_multi
    _C.swap_multi = lambda *a: (calls.append(1), real(*a))[1]
    try:
        for _ in range(2):
            epoch = pair_bottleneck._WEIGHTS_EPOCH[0]
            with avg.applied(model):
                assert pair_bottleneck._WEIGHTS_EPOCH[0] == epoch + 1
                assert all(_same(p, m) for p, m in zip(model.w, mean)) and all(_same(e, r) for e, r in zip(avg.tensors.values(), raw))
            assert pair_bottleneck._WEIGHTS_EPOCH[0] == epoch + 2
            assert all(_same(p, r) for p, r in zip(model.w, raw)) and all(_same(e, m) for e, m in zip(avg.tensors.values(), mean))
    finally:
        _C.swap_multi = real
    assert len(calls) == 4   # one launch in, one out
    assert pointers == [(p.data_ptr(), e.data_ptr()) for p, e in zip(model.w, avg.tensors.values())]
    taken = []
    cached = opt._step_cached
    opt._step_cached = lambda groups, *w: (taken.append(cached(groups, *w)), taken[-1])[1]
    opt.step()
    assert taken == [True]   # values moved, pointers stayed: the optimizer's tables are still valid


# ---- 4. inside a training process ------------------------------------------------------------------------------------------------------
NAME = "tiny_other_val"
OTHER_CATEGORIES = [8, 44, 3]
SMALL = ["INPUT.MIN_SIZE_TRAIN", "(64, 96)", "INPUT.MAX_SIZE_TRAIN", "128", "INPUT.MIN_SIZE_TEST", "80", "INPUT.MAX_SIZE_TEST",
         "128", "SOLVER.IMS_PER_BATCH", "2", "TEST.IMS_PER_BATCH", "2", "MODEL.RPN.PRE_NMS_TOP_N_TRAIN", "300",
         "MODEL.RPN.PRE_NMS_TOP_N_TEST", "200", "MODEL.RPN.POST_NMS_TOP_N_TRAIN", "60", "MODEL.RPN.POST_NMS_TOP_N_TEST", "40",
         "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", "16"]
TRAINING = ["DATALOADER.NUM_WORKERS", 0, "SOLVER.CHECKPOINT_PERIOD", 2, "SOLVER.TEST_PERIOD", 2, "SOLVER.LOG_PERIOD", 1,
            "SOLVER.BASE_LR", 0.005, "SOLVER.WARMUP_ITERS", 0, "DATASETS.TEST", (NAME,)]
CONFIG = "zeroshot_mask"   # the teacher: trainable trunk stages, RPN and heads, pair-layout operands prepared behind the step
SEED = 1234


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same_tree(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same_tree(x, y) for x, y in zip(a, b))
    return a == b


def _same_predictions(got, want):
    if len(got) != len(want):
        return False
    for a, b in zip(got, want):
        if a.size != b.size or sorted(a.fields()) != sorted(b.fields()) or a.bbox.shape != b.bbox.shape:
            return False
        if not torch.equal(a.bbox.cpu(), b.bbox.cpu()):
            return False
        if not all(torch.equal(a.get_field(f).cpu(), b.get_field(f).cpu()) for f in a.fields()):
            return False
    return True


def _checkpoint(out, name):
    return torch.load(os.path.join(out, name), map_location="cpu", weights_only=False)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Four runs of 4 iterations from the same seeds -- plain; ``--ema``; ``--ema --evaluate``; ``--ema`` with an evaluator of the
    test's own behind iterations 2 and 4 that looks at the model outside and inside ``applied`` -- and
    ``tools/infer_net.py --ema --evaluate`` from the third run's final checkpoint."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.catalog import DatasetCatalog
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import evaluation, trainer
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.detector import build_detection_model

    paths = tiny_coco.write(tmp_path_factory.mktemp("tiny_model_ema"))
    with open(paths["instances"]) as f:
        data = json.load(f)
    by_id = {c["id"]: c for c in data["categories"]}
    data["categories"] = [by_id[c] for c in OTHER_CATEGORIES]
    data["annotations"] = [a for a in data["annotations"] if a["category_id"] in OTHER_CATEGORIES]
    with open(os.path.join(paths["root"], "instances_other.json"), "w") as f:
        json.dump(data, f)
    with open(paths["catalog"]) as f:
        catalog = json.load(f)
    catalog[NAME] = {"img_dir": "images", "ann_file": "instances_other.json"}
    with open(paths["catalog"], "w") as f:
        json.dump(catalog, f)

    root = tmp_path_factory.mktemp("runs_model_ema")
    out = {k: str(root / k) for k in ("plain", "ema", "ema_eval", "hooked", "infer")}
    tool = _tool("train_net")

    def train(key, **kwargs):
        torch.manual_seed(SEED)
        cfg = tiny_coco.small_cfg(CONFIG, extra=TRAINING + ["OUTPUT_DIR", out[key]])
        history = tool.train(cfg, 0, False, 4, 2, save_checkpoints=True, dataset_catalog=paths["catalog"],
                             data_dir=paths["root"], seed=5, **kwargs)
        torch.cuda.synchronize()
        return history

    res = {"out": out, "paths": paths}
    res["plain"] = train("plain")
    res["ema"] = train("ema", ema_decay=DECAY)
    res["ema_eval"] = train("ema_eval", ema_decay=DECAY, evaluate=True)

    seen = {}
    cat = DatasetCatalog(paths["catalog"], paths["root"])
    no_output = tiny_coco.small_cfg(CONFIG, extra=TRAINING + ["OUTPUT_DIR", ""])
    real_do_train = trainer.do_train

    def do_train(cfg, model, *args, **kwargs):
        ema = kwargs["ema"]

        def detect(net):
            modes = [(m, m.training) for m in net.modules()]
            embeddings = net.roi_heads["box"].predictor.cls_score
            device = embeddings.device
            host_rng, device_rng = torch.get_rng_state(), torch.cuda.get_rng_state(device)
            found = evaluation.run_datasets(no_output, net, cat, device)[NAME]
            for module, mode in modes:
                module.training = mode
            net.set_class_embeddings(embeddings)
            torch.set_rng_state(host_rng)
            torch.cuda.set_rng_state(device_rng, device)
            return found

        def evaluator(iteration):
            host_rng, device_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
            raw = detect(model)
            with ema.applied(model):
                averaged = detect(model)
                state = {k: v.detach().clone() for k, v in model.state_dict().items()}
            fresh = build_detection_model(no_output).to(model.roi_heads["box"].predictor.cls_score.device)
            fresh.load_state_dict(state)
            fresh.set_class_embeddings(model.roi_heads["box"].predictor.cls_score)
            seen[iteration] = {"raw": raw, "averaged": averaged, "fresh": detect(fresh), "updates": ema.num_updates,
                               "lag": max(float((state[k] - v).abs().max()) for k, v in model.state_dict().items())}
            del fresh
            torch.set_rng_state(host_rng)   # (building a model draws its initial weights)
            torch.cuda.set_rng_state(device_rng)
        return real_do_train(cfg, model, *args, **dict(kwargs, evaluator=evaluator, test_period=2))

    trainer.do_train = do_train   # (the tool calls ``trainer.do_train``)
    try:
        res["hooked"] = train("hooked", ema_decay=DECAY)
    finally:
        trainer.do_train = real_do_train
    res["seen"] = seen
    yaml = os.path.join(ROOT, f"configs/coco_cap_det/{CONFIG}.yaml")
    _tool("infer_net").main(["--config-file", yaml, "--dataset-catalog", paths["catalog"], "--data-dir", paths["root"],
                            "--evaluate", "--ema", "--ckpt", os.path.join(out["ema_eval"], "model_final.pth")] + SMALL +
                           ["DATALOADER.NUM_WORKERS", "0", "DATASETS.TEST", f"('{NAME}',)", "OUTPUT_DIR", out["infer"]])
    return res


def test_inside_applied_the_model_computes_with_the_averaged_weights_on_every_route(runs):
    """The stale-operand test: the pair-layout operands prepared behind the last optimizer step were made from the raw
    weights; served inside the context they would give the raw model's detections."""
    assert sorted(runs["seen"]) == [2, 4]
    for k in (2, 4):
        seen = runs["seen"][k]
        assert seen["updates"] == k and seen["lag"] > 0
        assert sum(len(p) for p in seen["averaged"]) > 0
        assert _same_predictions(seen["averaged"], seen["fresh"]), k
        assert not _same_predictions(seen["averaged"], seen["raw"]), k
    assert not _same_predictions(runs["seen"][2]["averaged"], runs["seen"][4]["averaged"])


def test_training_goes_on_behind_the_context_as_if_it_had_not_been_entered(runs):
    out = runs["out"]
    assert [i for i, _ in runs["ema"]][-3:] == [2, 3, 4]
    assert all(v == v and abs(v) < 1e6 for _, losses in runs["ema"] for v in losses.values())
    # iterations 3 and 4 follow an ``applied`` behind iteration 2: same losses, and the same weights, momentum and averages
    assert _same_tree(runs["hooked"], runs["ema"]) and _same_tree(runs["ema_eval"], runs["ema"])
    for name in ("model_0000002.pth", "model_0000004.pth", "model_final.pth"):
        want = _checkpoint(out["ema"], name)
        assert list(want) == ["model", "optimizer", "scheduler", "iteration", "ema"]
        assert _same_tree(_checkpoint(out["hooked"], name), want), name
        assert _same_tree(_checkpoint(out["ema_eval"], name), want), name
    first, last = _checkpoint(out["ema"], "model_0000002.pth"), _checkpoint(out["ema"], "model_final.pth")
    assert first["ema"]["num_updates"] == 2 and last["ema"]["num_updates"] == 4
    assert not _same_tree(first["ema"]["params"], last["ema"]["params"]) and not _same_tree(first["model"], last["model"])
    trainable = list(last["ema"]["params"])
    assert trainable and all(not _same_tree(last["ema"]["params"][k], last["model"][k]) for k in trainable)


def test_raw_weights_and_momentum_equal_a_run_without_the_flag(runs):
    out = runs["out"]
    assert _same_tree(runs["plain"], runs["ema"])
    for name in ("model_0000002.pth", "model_0000004.pth", "model_final.pth"):
        plain, averaged = _checkpoint(out["plain"], name), _checkpoint(out["ema"], name)
        assert list(plain) == ["model", "optimizer", "scheduler", "iteration"]
        for k in plain:
            assert _same_tree(plain[k], averaged[k]), (name, k)
    assert not os.path.exists(os.path.join(out["plain"], "inference_ema"))
    assert not os.path.exists(os.path.join(out["ema"], "inference_ema")) and not os.path.exists(os.path.join(out["ema"], "inference"))


def test_inference_ema_holds_the_averaged_results_and_inference_the_raw_ones(runs):
    out = runs["out"]["ema_eval"]
    raw_dir, ema_dir = os.path.join(out, "inference", NAME), os.path.join(out, "inference_ema", NAME)
    assert sorted(os.listdir(raw_dir)) == ["coco_results.json", "predictions.pth"]
    assert sorted(os.listdir(ema_dir)) == ["coco_results.json", "coco_results_0000002.json", "coco_results_0000004.json",
                                           "predictions.pth"]
    raw = torch.load(os.path.join(raw_dir, "predictions.pth"), weights_only=False)
    averaged = torch.load(os.path.join(ema_dir, "predictions.pth"), weights_only=False)
    # max_iter is 4: the final weights are iteration 4's, and the other run looked at them outside and inside the context
    assert _same_predictions(raw, runs["seen"][4]["raw"]) and _same_predictions(averaged, runs["seen"][4]["averaged"])
    with open(os.path.join(ema_dir, "coco_results.json")) as f, open(os.path.join(ema_dir, "coco_results_0000004.json")) as g:
        final = json.load(f)
        assert final == json.load(g) and list(final) == ["bbox", "segm"]
    # tools/infer_net.py --ema: a freshly built model, the checkpoint's averages -> the same detections, under inference_ema/
    folder = os.path.join(runs["out"]["infer"], "inference_ema", NAME)
    assert sorted(os.listdir(folder)) == ["coco_results.json", "predictions.pth"]
    assert not os.path.exists(os.path.join(runs["out"]["infer"], "inference"))
    assert _same_predictions(torch.load(os.path.join(folder, "predictions.pth"), weights_only=False), averaged)
    with open(os.path.join(folder, "coco_results.json")) as f:
        assert json.load(f) == final
