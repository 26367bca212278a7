"""CPU: ``--lvis`` on the command lines -- valid only with ``--evaluate`` on tools/infer_net.py and tools/train_net.py, accepted
by tools/score_results.py -- and the names LVIS-style numbers are written under."""
import importlib.util
import os

import pytest

from tests import tiny_lvis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("tool", ["infer_net", "train_net"])
def test_lvis_without_evaluate_is_a_command_line_error(tool, tmp_path, capsys):
    argv = ["--lvis", "--dataset-catalog", str(tmp_path / "none.json"), "MODEL.DEVICE", "cuda", "OUTPUT_DIR", str(tmp_path)]
    with pytest.raises(SystemExit) as e:
        _tool(tool).main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--lvis" in err and "only with --evaluate" in err, err
    # beside the other scoring switches the message is still --lvis' own
    with pytest.raises(SystemExit) as e:
        _tool(tool).main(["--boundary-ap"] + argv)
    assert e.value.code == 2 and "--lvis" in capsys.readouterr().err


def test_score_results_accepts_lvis(tmp_path, capsys):
    ann = tiny_lvis.write(tmp_path / "lvis.json")
    (tmp_path / "bbox.json").write_text("[]")
    (tmp_path / "segm.json").write_text("[]")
    score = _tool("score_results")
    # the flag parses, alone and beside --boundary-ap and --recall: the next error is the device's, not the flag's
    for extra in ([], ["--boundary-ap", "--recall"]):
        with pytest.raises(SystemExit) as e:
            score.main(["--ann-file", ann, "--results-dir", str(tmp_path), "--lvis", "--device", "cpu"] + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "HIP device" in err and "unrecognized" not in err, err
    with pytest.raises(SystemExit):
        score.main(["--ann-file", ann, "--results-dir", str(tmp_path), "--lvis=300", "--device", "cpu"])   # a switch: no value
    assert "--lvis" in capsys.readouterr().err


def test_lvis_numbers_are_written_under_their_own_names():
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import evaluation
    assert evaluation.results_file_name() == "coco_results.json" and evaluation.results_file_name(False, 12) == "coco_results_0000012.json"
    assert evaluation.results_file_name(True) == "lvis_results.json" and evaluation.results_file_name(True, 12) == "lvis_results_0000012.json"


def test_the_rule_text_is_in_the_header_and_the_docs():
    with open(os.path.join(ROOT, "include", "ovis_hip.h")) as f:
        header = f.read()
    assert "ovis_lvis_match" in header and "neg_category_ids" in header and "not_exhaustive_category_ids" in header
    for name in ("README.md", "DESIGN.md"):
        with open(os.path.join(ROOT, name)) as f:
            text = " ".join(f.read().split())
        assert "lvis-api" in text and "not been compared with lvis-api" in text, name
