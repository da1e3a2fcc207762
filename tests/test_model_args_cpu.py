"""CPU: every refusal that stg_model_fwd, stg_model_bwd, stg_model_bwd_nll, stg_model_bwd_step and stg_model_step answer
ahead of their first HIP runtime call -- status and stg_last_error text -- against tests/model_refusals.json, the answers
of the library built from commit 7703007, the last one before the call records of csrc/step_plan.hpp
(tools/record_model_refusals.py holds the cases and recorded the table).  The order in which an entry point refuses is
ABI behaviour: ops.py tells the silent STG_EUNSUPPORTED returns, which leave the message alone, from errors."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_model_refusals",
                                                  os.path.join(ROOT, "tools", "record_model_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _recorder()
TABLE = json.load(open(os.path.join(ROOT, "tests", "model_refusals.json")))["rows"]


@pytest.fixture(scope="module")
def H():
    from social_stgcnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return R.bind(_lib.LIB_PATH)


def test_the_table_holds_the_recorders_cases_and_only_refusals():
    """The recorded rows are the recorder's cases, in its order; every row is a refusal (or the empty forward's STG_OK),
    so replaying it launches nothing; the cases the issue names are there."""
    assert [{k: v for k, v in r.items() if k not in ("status", "message")} for r in TABLE] == R.cases()
    ids = [r["id"] for r in TABLE]
    assert len(set(ids)) == len(ids)
    for r in TABLE:
        assert r["status"] in R.STATUSES or (r["status"] == 0 and r["id"] == "model_fwd: N = 0, every pointer null"), r["id"]
    # the answers that leave stg_last_error as the call before them left it: the empty forward and the silent refusals
    silent = {r["id"]: r["status"] for r in TABLE if r["message"] == R.SENTINEL}
    assert silent == {"model_fwd: N = 0, every pointer null": 0, "model_bwd_nll: SPLIT_BF16 (no message)": -2,
                      "model_bwd_nll: n_txpcnn = 0 (no message)": -2, "model_bwd_step: N = 0 (no message)": -2,
                      "model_step: N = 0 (no message)": -2, "model_step: SPLIT_BF16 (no message)": -2}
    assert sum(1 for r in TABLE if r["status"] == -3) == 3 and all("V = 400" in r["id"] for r in TABLE if r["status"] == -3)


@pytest.mark.parametrize("row", TABLE, ids=[r["id"] for r in TABLE])
def test_refusal_matches_the_recorded_answer(H, row):
    case = {k: v for k, v in row.items() if k not in ("status", "message")}
    assert R.run_case(H, case) == (row["status"], row["message"])
