"""CPU: ``--error-analysis`` on the command lines -- valid only with ``--evaluate`` on tools/infer_net.py, never with ``--lvis``,
a plain switch that is off by default and leaves every other option as it was -- and the places the rule text must be in."""
import argparse
import importlib.util
import os

import pytest

from tests import tiny_coco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}_errors", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fails(tool, argv, capsys):
    with pytest.raises(SystemExit) as e:
        _tool(tool).main(argv)
    assert e.value.code == 2
    return " ".join(capsys.readouterr().err.split())


def test_error_analysis_without_evaluate_is_a_command_line_error(tmp_path, capsys):
    tail = ["--dataset-catalog", str(tmp_path / "none.json"), "MODEL.DEVICE", "cuda", "OUTPUT_DIR", str(tmp_path)]
    err = _fails("infer_net", ["--error-analysis"] + tail, capsys)
    assert "--error-analysis" in err and "only with --evaluate" in err, err
    err = _fails("infer_net", ["--error-analysis", "--boundary-ap"] + tail, capsys)   # beside another scoring switch: its own message
    assert "--error-analysis" in err and "only with --evaluate" in err, err


def test_error_analysis_with_lvis_is_a_command_line_error(tmp_path, capsys):
    tail = ["--dataset-catalog", str(tmp_path / "none.json"), "MODEL.DEVICE", "cuda", "OUTPUT_DIR", str(tmp_path)]
    err = _fails("infer_net", ["--evaluate", "--lvis", "--error-analysis"] + tail, capsys)
    assert "--error-analysis" in err and "does not go with --lvis" in err, err
    ann = tiny_coco.write(tmp_path / "data")["instances"]
    (tmp_path / "bbox.json").write_text("[]")
    err = _fails("score_results", ["--ann-file", ann, "--results-dir", str(tmp_path), "--lvis", "--error-analysis"], capsys)
    assert "--error-analysis" in err and "does not go with --lvis" in err, err


def test_score_results_accepts_the_switch(tmp_path, capsys):
    ann = tiny_coco.write(tmp_path / "data")["instances"]
    (tmp_path / "bbox.json").write_text("[]")
    # the flag parses, alone and beside --boundary-ap's neighbours: the next error is the device's, not the flag's
    for extra in ([], ["--recall"]):
        err = _fails("score_results", ["--ann-file", ann, "--results-dir", str(tmp_path), "--error-analysis", "--device", "cpu"] + extra,
                     capsys)
        assert "HIP device" in err and "unrecognized" not in err, err
    err = _fails("score_results", ["--ann-file", ann, "--results-dir", str(tmp_path), "--error-analysis=0.5", "--device", "cpu"], capsys)
    assert "--error-analysis" in err   # a switch: no value, the thresholds have no command-line form


def test_the_flag_absent_leaves_every_other_option_as_it_was(tmp_path, monkeypatch, capsys):
    seen = []
    real = argparse.ArgumentParser.parse_args

    def spy(self, *a, **k):
        seen.append(real(self, *a, **k))
        return seen[-1]
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", spy)
    tail = ["--dataset-catalog", str(tmp_path / "none.json"), "MODEL.DEVICE", "cpu"]   # --evaluate stops there: no host scoring
    _fails("infer_net", ["--evaluate", "--recall"] + tail, capsys)
    _fails("infer_net", ["--evaluate", "--recall", "--error-analysis"] + tail, capsys)
    off, on = vars(seen[0]), vars(seen[1])
    assert off.pop("error_analysis") is False and on.pop("error_analysis") is True and off == on
    assert sorted(off) == ["bbox_vote", "boundary_ap", "ckpt", "config_file", "data_dir", "dataset_catalog", "evaluate",
                           "export_results", "local_rank", "lvis", "mask_aug", "opts", "recall", "rpn_recall", "vis_threshold",
                           "visualize"]
    assert off["evaluate"] and off["recall"] and not off["lvis"] and off["opts"] == ["MODEL.DEVICE", "cpu"]
    ann = tiny_coco.write(tmp_path / "data")["instances"]
    (tmp_path / "bbox.json").write_text("[]")
    del seen[:]
    _fails("score_results", ["--ann-file", ann, "--results-dir", str(tmp_path), "--device", "cpu"], capsys)
    args = vars(seen[0])
    assert args.pop("error_analysis") is False
    assert sorted(args) == ["ann_file", "bbox", "boundary_ap", "device", "lvis", "output", "recall", "results_dir", "segm"]


def test_run_datasets_refuses_the_analysis_without_evaluate_or_with_lvis():
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import evaluation
    with pytest.raises(ValueError, match="error_analysis"):
        evaluation.run_datasets(None, None, None, "cuda", error_analysis=True)
    with pytest.raises(ValueError, match="error_analysis"):
        evaluation.run_datasets(None, None, None, "cuda", evaluate=True, lvis=True, error_analysis=True)
    with pytest.raises(ValueError, match="COCO's rules"):
        evaluation.save_evaluation(None, None, None, ("bbox",), "cuda", None, lvis=True, errors=True)


def test_the_rule_text_is_in_the_header_and_the_docs():
    with open(os.path.join(ROOT, "include", "ovis_hip.h")) as f:
        header = " ".join(f.read().replace(" * ", " ").split())
    for phrase in ("ovis_error_types", "t_b <= s < t_f", "max(s, o) <= t_b", "An equal IoU goes to the later ground-truth row",
                   "ties going to the earlier detection row", "dAP50_<T>_split_<split>", "NOT been compared with tidecv"):
        assert phrase in header, phrase
    for name in ("README.md", "DESIGN.md"):
        with open(os.path.join(ROOT, name)) as f:
            text = " ".join(f.read().split())
        assert "tidecv" in text and "--error-analysis" in text and "not been compared with tidecv" in text, name
