"""What tests/context_order rests on, checked without a GPU: every entry point that uses the workspace arena has a probe,
the ladder's needs grow as the growth test says, the seeded queues are fixed, and the fill hook is declared as the tests
use it (tests/context_order_inputs.py)."""
import hashlib
import os
import re

import context_order_inputs as co

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gps-jamming_amd", "csrc")


def test_every_workspace_user_has_a_probe():
    """Every function of csrc/*.hip and *.h that calls ensure_workspace or names ctx->ws is in the table, the table
    resolves it to its extern "C" entry points, and each of those has a probe (or is exempt, with the reason).  A new user
    of the arena turns this red until it has a probe."""
    found = co.workspace_users(CSRC)
    assert found, "no workspace user found: the scan is broken"
    assert sorted(found) == sorted(co.WORKSPACE_USERS), (sorted(set(found) ^ set(co.WORKSPACE_USERS)), found)
    probed = {e for s in co.SPECS.values() for e in s.entries}
    header = open(os.path.join(REPO, "include", "gpsjam.h")).read()
    for fn, entries in co.WORKSPACE_USERS.items():
        for e in entries:
            assert re.search(r"\b%s\(" % e, header), f"{e} (reached from {fn}) is not an entry point of include/gpsjam.h"
            assert e in probed or e in co.EXEMPT, f"{e} uses the workspace (through {fn}) and has no probe"
    assert set(co.EXEMPT) == {"gj_reserve"} and all(len(r) > 20 for r in co.EXEMPT.values())
    assert not set(co.EXEMPT) & probed
    # every probe is in the catalogue of the tests that take "all of them", and only the self-synchronising one is kept
    # out of the queues that must not wait
    assert set(co.SMALL) | set(co.LADDER) == set(co.SPECS)
    assert [n for n in co.SMALL if n not in co.QUEUED] == ["welch_timed"]


def test_the_scan_sees_a_use_that_the_table_does_not_know(tmp_path):
    """The coverage test can fail: a made-up kernel file with a new caller."""
    (tmp_path / "k_new.hip").write_text("namespace gj {\nint launch_new(gj_ctx* ctx, size_t n) {\n    int rc = ensure_workspace(ctx, n);\n"
                                        "    float* p = reinterpret_cast<float*>(ctx->ws);   // scratch\n    return rc;\n}\n}\n"
                                        "int ensure_workspace(gj_ctx* ctx, size_t bytes);\n// ctx->ws in a comment\n")
    assert co.workspace_users(str(tmp_path)) == {"launch_new": ["k_new.hip:3", "k_new.hip:4"]}


def test_the_ladder_on_the_cpu():
    """The ladder's probes all state their need through functions that answer without a context (the kurtosis, K5, the CAF
    and the series; K2's needs one and is no rung), so the inequality the growth test asserts on the device holds here too."""
    needs = [co.SPECS[n].need(None) for n in co.LADDER]
    assert all(isinstance(x, int) for x in needs), needs
    assert co.ladder_holds(needs) == [], needs
    assert co.ladder_holds([co.MiB, 4 * co.MiB - 1]) == [(0, co.MiB, 4 * co.MiB - 1)]
    assert len(co.LADDER) >= 6 and len({co.LADDER_KERNELS[n] for n in co.LADDER}) >= 4
    assert co.MiB <= needs[0] < 2 * co.MiB and needs[-1] <= 256 * co.MiB
    assert needs == sorted(needs)


def test_the_seeded_queues_are_fixed():
    assert len(co.QUEUE_SEEDS) == len(set(co.QUEUE_SEEDS)) == 8
    orders = set()
    for seed in co.QUEUE_SEEDS:
        q = co.seeded_queue(seed)
        assert q == co.seeded_queue(seed)
        names = [n for n, _, _ in q]
        assert sorted(names) == sorted(co.QUEUED * 2)
        for n in co.QUEUED:                                    # first place: slot 0, second place: slot 1
            assert [slot for m, slot, _ in q if m == n] == [0, 1]
        fills = [b for _, _, b in q if b is not None]
        assert len(set(fills)) == 1 and fills[0] in co.FILLS and len(fills) in (len(q) // 3, len(q) // 3 + 1)
        orders.add(tuple(names))
    assert len(orders) == 8
    digest = [hashlib.sha256(repr(co.seeded_queue(s)).encode()).hexdigest()[:16] for s in co.QUEUE_SEEDS[:2]]
    assert digest == ["22c1f32dd79250b2", "033beb24681c1889"], digest


def test_the_fill_hook_is_declared_as_the_tests_use_it():
    header = open(os.path.join(REPO, "include", "gpsjam.h")).read()
    assert re.search(r"#define GJ_INJECT_FILL_WORKSPACE %d\b" % co.GJ_INJECT_FILL_WORKSPACE, header)
    assert re.search(r"#define GJ_INJECT_OWNER_ALIVE 1\b", header)
    stub = open(os.path.join(REPO, "tests", "hip_stub", "san_scenarios.cpp")).read()
    assert "GJ_INJECT_FILL_WORKSPACE" in stub[stub.index("scenario_workspace"):stub.index("scenario_workspace") + 5000]
    assert co.FILLS == (0x00, 0xFF, 0x7F) and co.CONVENTIONS[:2] == ((127.5, 1.0 / 127.5), (128.0, 1.0 / 128.0))


def test_the_convention_probes_cover_the_offset_honouring_kernels():
    layouts = {co.SPECS[n].entries[0] for n in co.CONVENTION_PROBES}
    assert layouts == {"gj_chunk_power_dev", "gj_capture_scan_dev", "gj_welch_dev", "gj_xcorr_lags_dev", "gj_xcorr_caf_dev", "gj_sk_dev",
                       "gj_csd_dev"}
    assert all(co.SPECS[n].honours_unpack for n in co.CONVENTION_PROBES) and not co.SPECS[co.FIXED_128_PROBE].honours_unpack
