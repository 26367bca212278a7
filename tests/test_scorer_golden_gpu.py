"""GPU: the scorer (engine/coco_eval.py) against the commit before it was restructured -- every array of every match table
of tests/golden/make_scorer_golden.py's configurations equals what that commit gave on the device
(tests/golden/scorer_tables.npz), error arrays included, as one chunk and in chunks of one image; and a chunk makes the same
``_C`` calls in the same order (tests/golden/scorer_calls.json)."""
import json

import numpy as np
import pytest

from tests.golden import make_scorer_golden as golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scored():
    return golden.score_all("cuda")


def test_every_table_equals_the_recorded_one(scored):
    arrays, _ = scored
    with np.load(golden.TABLES_FILE) as want:
        assert sorted(arrays) == sorted(want.files)
        assert {key.split("/")[0] for key in arrays} == {name for name, _, _, _ in golden.CONFIGS} and len(golden.CONFIGS) == 14
        for key in want.files:
            assert arrays[key].dtype == want[key].dtype and np.array_equal(arrays[key], want[key]), key
        assert any(key.endswith("/err_type") for key in want.files) and any("_lvis/per_image/boundary/" in key for key in want.files)


def test_a_chunk_makes_the_recorded_calls_in_the_recorded_order(scored):
    _, calls = scored
    with open(golden.CALLS_FILE) as f:
        want = json.load(f)
    assert sorted(calls) == sorted(want)
    for name in want:
        assert calls[name] == want[name], name
