"""The GPU suite runs core-first (tests/conftest.py SUITE_ORDER): the driver's `pytest -x -m gpu` must reach the oracle
parity tests of K1-K5 and of the BASELINE configs before anything that spawns processes or kills threads, so that one
peripheral failure cannot hide the hot path (GPUTEST_r04: red at test 15 of 374, 359 unreached).  Ordering only --
nothing may be deselected, skipped or expected to fail.

No test module is another's library: what two of them share stands in a module that holds no tests (tests/gpu_lib.py,
tests/host_lib.py, the restatements and inputs), so that editing a test file changes what that file asserts and nothing else."""
import ast
import os
import re
import subprocess
import sys

import conftest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def collected(marker):
    out = subprocess.run([sys.executable, "-m", "pytest", "tests", "-m", marker, "--collect-only", "-q", "-p", "no:cacheprovider"],
                         cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return [ln.strip() for ln in out.stdout.splitlines() if "::" in ln]


def test_gpu_suite_runs_parity_first_and_thread_killers_last():
    ids = collected("gpu")
    assert len(ids) >= 374
    files = []
    for i in ids:
        f = i.split("::")[0].split("/")[-1]
        if not files or files[-1] != f:
            files.append(f)
    assert len(files) == len(set(files)), f"a file's tests are not contiguous: {files}"
    assert files[0] == "test_gpu_parity.py"
    assert files[1] == "test_baseline_configs_gpu.py"
    assert ids[-1].endswith("test_c_abi_gpu.py::test_abandoned_callers_do_not_block_the_context")
    # every file with GPU tests has a place in the order, and the order is the one declared
    assert [f for f in files if f not in conftest.SUITE_ORDER] == []
    assert files == [f for f in conftest.SUITE_ORDER if f in files]
    # the hot path's parity files all come before the first file that spawns processes or kills threads
    pos = {f: k for k, f in enumerate(files)}
    core = ["test_gpu_parity.py", "test_baseline_configs_gpu.py", "test_dropin_modules.py", "test_extremes_gpu.py",
            "test_gpu_random_sweep.py", "test_large_capture_gpu.py"]
    peripheral = ["test_sharded_two_rank_gpu.py", "test_bench_launch.py", "test_errors_gpu.py", "test_threads_gpu.py", "test_c_abi_gpu.py"]
    assert max(pos[f] for f in core) < min(pos[f] for f in peripheral)
    # BASELINE configs[1]'s own test (1 GiB through K2 at nperseg 4096) is among the first tenth of the run
    full = [k for k, i in enumerate(ids) if "test_full_size_1gib_properties" in i]
    assert full and full[0] < len(ids) // 3


def test_nothing_is_skipped_or_expected_to_fail():
    pat = re.compile(r"pytest\.mark\.(skip|skipif|xfail)|pytest\.(skip|xfail)\(|importorskip")
    me = os.path.basename(__file__)
    hits = []
    for f in sorted(os.listdir(os.path.join(REPO, "tests"))):
        if f.endswith(".py") and f != me:
            for n, line in enumerate(open(os.path.join(REPO, "tests", f)), 1):
                if pat.search(line):
                    hits.append(f"{f}:{n}: {line.strip()}")
    # three environmental skips predate the ordering and stay as they are: a busy TCP port on the host, a GPU without
    # room for a 5-GiB capture (never the case on an MI355X), and a CPU-only check that steps aside when a GPU is there
    allowed = {'test_dropin_modules.py': 'pytest.skip("port 1234 busy")',
               'test_large_capture_gpu.py': 'pytest.skip("needs a GPU with room for a 5 GiB capture")',
               'test_library_abi.py': 'pytest.skip("GPU present")'}
    hits = [h for h in hits if allowed.get(h.split(":")[0]) != h.split(": ", 1)[1]]
    assert hits == [], hits


def test_cpu_suite_is_unchanged_by_the_ordering():
    ids = collected("not gpu")
    assert len(ids) >= 92
    files = []
    for i in ids:
        f = i.split("::")[0].split("/")[-1]
        if not files or files[-1] != f:
            files.append(f)
    assert files == sorted(files), "CPU tests keep pytest's default (alphabetical by file) order"


def test_no_module_imports_a_test_module():
    """Every .py under tests/, imports inside functions included."""
    hits = []
    for root, _, names in os.walk(os.path.join(REPO, "tests")):
        for f in sorted(n for n in names if n.endswith(".py")):
            path = os.path.join(root, f)
            for node in ast.walk(ast.parse(open(path).read(), path)):
                if isinstance(node, ast.Import):
                    mods = [a.name for a in node.names]
                elif isinstance(node, ast.ImportFrom):
                    mods = [node.module or ""] + [f"{node.module or ''}.{a.name}" for a in node.names]
                else:
                    continue
                hits += [f"{os.path.relpath(path, REPO)}:{node.lineno}: {m}" for m in mods if any(p.startswith("test_") for p in m.split("."))]
    assert hits == [], hits
