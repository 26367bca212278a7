"""CPU: evaluation while training (SOLVER.TEST_PERIOD) -- when ``engine.trainer.do_train`` calls its ``evaluator``, the NumPy
merge of per-rank match tables behind ``engine.coco_eval.evaluate_coco_sharded``, and the command-line errors of
``tools/train_net.py --evaluate``.  What an evaluation does to a live training process is tests/test_train_eval_gpu.py's."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import coco_eval_reference as ref
from tests import tiny_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_KEYS = ("category", "det_start", "gt_start", "scores", "dt_match", "dt_ignore", "gt_ignore")


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the schedule ------------------------------------------------------------------------------------------------------------
class _Checkpointer:
    """Stands in for the checkpointer: records what it is asked to save."""

    def __init__(self, events):
        self.events = events

    def save(self, name, **extra):
        self.events.append(("save", name, extra.get("iteration")))


@pytest.fixture(scope="module")
def tiny():
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import model_cfg

    model, e_vocab, e_seen, images, targets = tiny_model.build_tiny("zeroshot_mask", batch=1)
    model.set_class_embeddings(e_seen)
    return model_cfg(model), copy.deepcopy(model.state_dict()), model, images, targets


def _run(tiny, monkeypatch, max_iter, start_iter=0, **kwargs):
    """``do_train`` from the same weights every time -> (history, events): a ("save", name, iteration) per checkpoint, an
    ("evaluate", iteration, live look-ahead workers, model.training inside the callable) per evaluator call."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import solver, trainer

    cfg, state, model, images, targets = tiny
    model.load_state_dict(copy.deepcopy(state))
    model.train()
    optimizer = solver.make_optimizer(cfg, model)
    events, pipes = [], []

    class Recorded(trainer.PipelinedTrainer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            pipes.append(self)

    monkeypatch.setattr(trainer, "PipelinedTrainer", Recorded)

    def evaluator(iteration):
        (pipe,) = pipes
        events.append(("evaluate", iteration, pipe.worker is not None and pipe.worker.is_alive(), model.training))
        model.eval()   # what an evaluation does ...
        model.train()  # ... and what it owes the loop

    if kwargs.pop("with_evaluator", True):
        kwargs["evaluator"] = evaluator
    history = trainer.do_train(cfg, model, iter([(images, targets)] * (max_iter - start_iter)), optimizer, None, max_iter,
                               start_iter=start_iter, log_period=1, checkpointer=_Checkpointer(events), checkpoint_period=2,
                               **kwargs)
    assert model.training
    return history, events


def test_do_train_calls_the_evaluator_every_test_period_behind_the_checkpoint(tiny, monkeypatch):
    history, events = _run(tiny, monkeypatch, 5, test_period=2)
    assert [i for i, _ in history] == [1, 2, 3, 4, 5]
    # iterations 2 and 4, each behind the save of the same iteration; no look-ahead worker alive, the model in training mode
    assert events == [("save", "model_0000002", 2), ("evaluate", 2, False, True), ("save", "model_0000004", 4),
                      ("evaluate", 4, False, True), ("save", "model_final", 5)]
    # the count is the run's, not the process': resumed behind iteration 2, the next evaluation is at 4
    _, resumed = _run(tiny, monkeypatch, 5, start_iter=2, test_period=2)
    assert [e for e in resumed if e[0] == "evaluate"] == [("evaluate", 4, False, True)]
    assert [e[1] for e in resumed if e[0] == "save"] == ["model_0000004", "model_final"]
    # no period, or no evaluator: no call, and the losses of a run that was not given the arguments at all
    plain, plain_events = _run(tiny, monkeypatch, 5, with_evaluator=False)
    saves = [e for e in events if e[0] == "save"]
    assert plain_events == saves
    for kwargs in (dict(test_period=0), dict(test_period=2, evaluator=None, with_evaluator=False)):
        again, again_events = _run(tiny, monkeypatch, 5, **kwargs)
        assert again_events == saves and again == plain
    assert history == plain  # the stand-in evaluator leaves the run alone


# ---- 2. the merge ---------------------------------------------------------------------------------------------------------------
def _images():
    """Five images for the restatement, three categories: equal scores across images (.9 in images 0, 2 and 4, category 0),
    an image with detections only, one with ground truth only, one with neither (it has no problem at all)."""
    gt = {"category": 0, "bbox": [10, 10, 20, 20], "area": 400.0, "iscrowd": 0}

    def det(bbox, score, category=0):
        return {"category": category, "bbox": bbox, "score": score}
    return [
        {"dets": [det([10, 10, 20, 20], .9), det([50, 50, 20, 20], .9), det([60, 60, 30, 30], .5, 1)],
         "gts": [gt, dict(gt, category=1, bbox=[60, 60, 30, 30], area=900.0)]},
        {"dets": [det([0, 0, 10, 10], .7, 2)], "gts": []},
        {"dets": [det([10, 10, 20, 12.5], .9), det([10, 10, 20, 20], .8)], "gts": [gt, dict(gt, iscrowd=1, bbox=[0, 0, 100, 100],
                                                                                              area=10000.0)]},
        {"dets": [], "gts": []},
        {"dets": [det([12, 10, 20, 20], .9)], "gts": [gt, dict(gt, category=2, bbox=[0, 0, 40, 40], area=1600.0)]},
    ]


def _shard(images, image_ids, members):
    """The restatement's tables of ``members`` (positions in ``images``), scored in THAT order, with the image id of every
    problem -- what a rank that predicted those images sends."""
    tables = ref.match_tables([images[k] for k in members], "bbox")
    counts = [len({d["category"] for d in images[k]["dets"]} | {g["category"] for g in images[k]["gts"]}) for k in members]
    tables["image"] = np.repeat(np.asarray([image_ids[k] for k in members], dtype=np.int64), counts)
    return tables


def test_merged_shard_tables_equal_the_unsharded_tables():
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval

    images, image_ids = _images(), [3, 8, 21, 40, 77]
    whole = ref.match_tables(images, "bbox")
    assert len(whole["category"]) == 6 and whole["scores"].tolist().count(.9) == 4
    # three shards by image, scrambled; image 21 (position 2) sits on ranks 0 and 2, rank 1 holds nothing
    shards = [_shard(images, image_ids, [4, 2, 0]), _shard(images, image_ids, []), _shard(images, image_ids, [2, 3, 1])]
    assert len(shards[1]["category"]) == 0 and 21 in shards[0]["image"] and 21 in shards[2]["image"]
    merged = coco_eval.merge_shard_tables(shards)
    assert sorted(merged) == sorted(TABLE_KEYS)
    for key in TABLE_KEYS:
        assert np.array_equal(merged[key], whole[key]), key
    assert np.array_equal(coco_eval.accumulate(merged, 3), coco_eval.accumulate(whole, 3))
    assert np.array_equal(coco_eval.accumulate(merged, 3), ref.accumulate(whole, 3))
    # the lowest rank's block is the one that is kept: rank 2's copy of image 21 may hold anything
    shards[2]["scores"] = shards[2]["scores"] * 0 + .123
    shards[2]["dt_match"] = shards[2]["dt_match"] * 0 - 1
    kept = dict(shards[2])
    again = coco_eval.merge_shard_tables(shards)
    first21, last21 = int(whole["det_start"][3]), int(whole["det_start"][4])   # problem 3 is image 21's
    assert last21 - first21 == 2 and not np.array_equal(again["scores"], whole["scores"])   # (image 8's row is rank 2's own)
    assert np.array_equal(again["scores"][first21:last21], whole["scores"][first21:last21])
    assert np.array_equal(again["dt_match"][:, :, first21:last21], whole["dt_match"][:, :, first21:last21])
    assert np.array_equal(kept["scores"], shards[2]["scores"])   # the parts are not written to
    # the same rule for dataset indices: the wrapped-around index 0 belongs to rank 0
    assert coco_eval.shard_owners([[0, 1, 2], [3, 4, 5], [6, 0]]) == {0: 0, 1: 0, 2: 0, 3: 1, 4: 1, 5: 1, 6: 2}
    assert coco_eval.shard_owners([[], [1], [1, 0]]) == {1: 1, 0: 2}
    with pytest.raises(ValueError):   # an image's problems are one block
        coco_eval.merge_shard_tables([dict(shards[0], image=np.asarray([77, 21, 77, 3, 3]))])
    empty = coco_eval.merge_shard_tables([shards[1]])
    assert len(empty["category"]) == 0 and empty["det_start"].tolist() == [0] and empty["dt_match"].shape == (4, 10, 0)


# ---- 3. the command line --------------------------------------------------------------------------------------------------------
def test_train_net_evaluate_is_a_command_line_error_without_catalog_output_dir_or_device(tmp_path, capsys):
    tool = _tool("train_net")
    catalog = ["--dataset-catalog", str(tmp_path / "none.json")]
    for argv, word in ((["--evaluate", "MODEL.DEVICE", "cuda", "OUTPUT_DIR", str(tmp_path)], "give --dataset-catalog"),
                       (["--evaluate"] + catalog + ["MODEL.DEVICE", "cuda", "OUTPUT_DIR", ""], "set OUTPUT_DIR"),
                       (["--evaluate"] + catalog + ["MODEL.DEVICE", "cpu", "OUTPUT_DIR", str(tmp_path)], "set MODEL.DEVICE cuda"),
                       (["--evaluate"] + catalog + ["MODEL.DEVICE", "cuda", "OUTPUT_DIR", str(tmp_path),
                                                    "TEST.BBOX_AUG.ENABLED", "True"], "set TEST.BBOX_AUG.ENABLED False")):
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert not os.listdir(tmp_path)


def test_train_refuses_evaluate_without_its_prerequisites(tmp_path):
    from tests import tiny_coco

    tool = _tool("train_net")
    cfg = tiny_coco.small_cfg(extra=["MODEL.DEVICE", "cpu", "OUTPUT_DIR", str(tmp_path)])
    with pytest.raises(ValueError, match="MODEL.DEVICE cuda"):
        tool.train(cfg, 0, False, 1, 1, dataset_catalog=str(tmp_path / "none.json"), evaluate=True)
