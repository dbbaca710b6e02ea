"""The step / reset dispatch (csrc/lbsim_plan.h make_plan) without a GPU: tests/plan_probe.cpp,
compiled as plain host C++, must give for every case of tests/golden/step_plan.jsonl the plan
recorded there.  The table was recorded from the predicates and launcher conditions the library
had before make_plan existed (dyn_group_lanes / dyn_wave_ok / use_step_wave / use_fused_step and
the launchers' own branches), on 256-CU and 104-CU devices, so a changed row is a changed
dispatch: re-record it only with the measurement that justifies the move.

The file: a header line (the probe's input fields with their defaults, the fields of a case, the
plan's fields), then blocks of a {"variant": {input field: value}} line and its cases, one
[simds, B, S, plan values...] per line."""
import json
import os
import subprocess

import pytest

from marllb_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def table(golden_dir):
    """(header, [(probe input row, recorded plan values)])"""
    with open(os.path.join(golden_dir, "step_plan.jsonl")) as f:
        head, *lines = [json.loads(line) for line in f]
    rows, variant = [], None
    for line in lines:
        if isinstance(line, dict):
            variant = line["variant"]
            continue
        inp = dict(zip(head["in"], head["defaults"]), **variant, **dict(zip(head["case"], line)))
        rows.append(([inp[k] for k in head["in"]], line[len(head["case"]):]))
    return head, rows


def run_probe(tmp, rows):
    """make_plan's answers to rows of 20 or 21 integers (the 21st: flow_stats), from plan_probe
    compiled into the directory tmp (once per directory)."""
    exe = str(tmp / "plan_probe")
    if not os.path.exists(exe):
        subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-o", exe,
                        os.path.join(HERE, "plan_probe.cpp")], check=True)
    text = "".join(" ".join(map(str, r)) + "\n" for r in rows)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    return [json.loads(line) for line in out.splitlines()]


@pytest.fixture(scope="module")
def probe_rows(table, tmp_path_factory):
    return run_probe(tmp_path_factory.mktemp("plan"), [inp for inp, _ in table[1]])


def _flat(plan):
    out = {}
    for k, v in plan.items():
        if isinstance(v, dict):
            out.update({f"{k}.{kk}": vv for kk, vv in v.items()})
        else:
            out[k] = v
    return out


def test_table_covers_the_dispatch(table):
    head, rows = table
    assert len(head["in"]) == 20 and len(rows) >= 600
    assert all(None not in inp and len(plan) == len(head["plan"]) for inp, plan in rows)
    col = {n: {plan[i] for _, plan in rows} for i, n in enumerate(head["plan"])}
    assert col["form"] == {0, 1, 2} and col["dynamics_kernel"] == {0, 1, 2}
    assert col["dyn.waves"] == {0, 1, 4, 5} and col["occ"] == {0, 2, 4}
    assert col["dyn.width"] == {1, 2, 4, 8, 16, 32, 64}
    assert col["obs.form"] == {0, 1, 2, 3, 5} and col["reset_obs.form"] == {3, 4, 5}
    servers = {inp[head["in"].index("S")] for inp, _ in rows}
    assert servers == {1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 24, 32, 33, 40, 64}


def test_make_plan_matches_recorded_dispatch(table, probe_rows):
    head, rows = table
    assert len(probe_rows) == len(rows)
    bad = []
    for (inp, want), got in zip(rows, probe_rows):
        got = _flat(got)
        assert list(got) == head["plan"]
        if list(got.values()) != want:
            diff = {n: (w, got[n]) for n, w in zip(head["plan"], want) if got[n] != w}
            bad.append((dict(zip(head["in"], inp)), diff))
    assert not bad, f"{len(bad)} cases differ (field: (recorded, got)); first: {bad[0]}"
