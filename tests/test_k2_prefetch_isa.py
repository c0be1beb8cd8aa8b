"""K2's prefetch in the GENERATED code (host test: cross-compiles k_welch.hip to gfx950 assembly, no GPU).

The carried front end (nperseg 4096 and 1024) asks for the next step's new half segment right behind the first LDS
scatter of a step and waits for it at the next step's unpack.  That was true of the source only: as plain loads the
compiler issued all eight behind the last butterfly of the step.  tools/k2_isa_report.py reads where they stand.

Threshold for "the loads are a whole pass ahead of their wait", from that report:
  before (plain loads)        58 (N = 4096) / 64 (N = 1024) vector-ALU instructions between the last sample load and
                              the s_waitcnt vmcnt(0) that covers it -- 78 / 82 instructions of every kind, the "about 70";
  one pass of the new kernel  92 (4096) / 93 (1024) vector-ALU instructions between two exchanges (about 120 of every kind);
  now                         270 (4096) / 231 (1024).
The test asks for at least one pass of the kernel as compiled (the report's own count, never fewer than 90).

It needs the compiler the library itself is built with and fails without it: this suite skips nothing
(test_suite_order.test_nothing_is_skipped_or_expected_to_fail)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ONE_PASS_AT_LEAST = 90
CHANGED = ("welch_kernel<4096,false>", "welch_kernel<4096,true>", "welch_kernel<1024,false>", "welch_kernel<1024,true>")


@pytest.fixture(scope="module")
def report():
    run = subprocess.run([sys.executable, os.path.join(REPO, "tools", "k2_isa_report.py"), "--json"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return json.loads(run.stdout)


def test_every_instantiation_is_reported(report):
    sizes = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
    assert set(report) == {f"welch_kernel<{n},{b}>" for n in sizes for b in ("false", "true")}
    for name, r in report.items():
        assert r["loop"] and r["loop"]["load_at"], name
        assert r["loop"]["last_load_to_wait"]["found"], name


@pytest.mark.parametrize("name", CHANGED)
def test_registers_scratch_occupancy(report, name):
    r = report[name]
    print(name, {k: r[k] for k in ("vgprs", "scratch", "occupancy")})
    assert r["scratch"] == 0
    assert r["vgprs"] <= 168
    assert r["occupancy"] == 3


@pytest.mark.parametrize("name", CHANGED)
def test_sample_loads_stand_behind_the_first_scatter(report, name):
    lp = report[name]["loop"]
    print(name, "loads at", lp["load_at"], "first scatter ends at", lp["first_scatter_ends_at"], lp["sync_kind"], "at", lp["sync_at"])
    assert lp["load_kinds"] == ["global_load_ushort"] and len(lp["load_at"]) == 8
    assert lp["sync_kind"] == ("s_barrier" if "<4096" in name else "wave fence") and len(lp["sync_at"]) == 4
    assert lp["loads_before_first_sync"]          # every sample load precedes the first exchange's barrier / fence
    assert lp["loads_behind_first_scatter"]       # ... and follows that exchange's scatter: the points are in LDS


@pytest.mark.parametrize("name", CHANGED)
def test_a_whole_pass_lies_between_the_last_load_and_its_wait(report, name):
    lp = report[name]["loop"]
    w = lp["last_load_to_wait"]
    print(name, "VALU in one pass", lp["valu_one_pass"], "last load -> wait", w)
    assert w["found"] and w["wait"].replace(" ", "") == "s_waitcntvmcnt(0)"
    assert lp["valu_one_pass"] >= ONE_PASS_AT_LEAST
    assert w["valu"] >= lp["valu_one_pass"]
    # the wait stays at the next step's unpack: in front of the step's first LDS write
    assert w["wait_at"] is not None and w["wait_at"] < lp["first_lds_write_at"]
