#!/usr/bin/env python3
"""Where K2's sample loads stand in the GENERATED code (no GPU needed).

Compiles gps-jamming_amd/csrc/k_welch.hip device-only to gfx950 assembly with exactly the flags the Makefile gives
that file (asked of `make -n`, not copied) and prints, for every welch_kernel instantiation:
  * VGPRs, scratch bytes and occupancy (the compiler's own summary);
  * for the steady-state loop (the largest loop of the kernel): where the global loads -- in that loop only the
    sample loads -- stand relative to the LDS exchanges' barriers / wave fences;
  * how many vector (VALU) instructions lie between the last sample load and the s_waitcnt vmcnt that covers it,
    followed along the loop's fall-through path and across its back edge.
  * for every block of that loop together: instructions, vector instructions, s_nop and branches.
It reads loads, waits, barriers, LDS instructions, mnemonics and the register summary, nothing else.

    python tools/k2_isa_report.py                 # the table
    python tools/k2_isa_report.py --json          # the same as JSON (tests/test_k2_prefetch_isa.py reads this)
    python tools/k2_isa_report.py --source k_ridge.hip --kernels ridge   # another file's kernels, e.g. the short-time front end
    python tools/k2_isa_report.py --source k_scan.hip --kernels stream_scan_kernel   # the fused scan (its loop: one full tile)
    python tools/k2_isa_report.py --asm FILE      # report on an assembly file made earlier (e.g. of another commit)
"""
import argparse
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gps-jamming_amd", "csrc")


def compile_command(source):
    """The Makefile's own command line for <source>'s object, turned into 'device-only, to assembly'."""
    obj = os.path.splitext(source)[0] + ".o"
    out = subprocess.run(["make", "-C", CSRC, "-n", "-W", source, obj], capture_output=True, text=True, check=True).stdout
    for line in out.splitlines():
        words = shlex.split(line)
        if "-c" in words and source in words and obj in words:
            words = [w for w in words if w not in ("-c", obj, "-o")]
            return words
    raise RuntimeError(f"the Makefile gives no compile command for {obj}:\n{out}")


def compile_to_asm(source, path):
    cmd = compile_command(source) + ["--cuda-device-only", "-S", "-o", path]
    subprocess.run(cmd, cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
    return cmd


_LABEL = re.compile(r"^([.\w$]+):")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")


def split_functions(text, name_re):
    """{mangled name: (instruction list, summary dict)}; an instruction is (mnemonic, operands, labels in front of it)."""
    funcs = {}
    cur = None
    pending = []
    for line in text.splitlines():
        m = _LABEL.match(line)
        if m and not line.startswith(".L") and cur is None and not m.group(1).endswith(".kd") and re.search(name_re, m.group(1)):
            cur = {"name": m.group(1), "ins": [], "summary": {}}
            pending = []
            continue
        if cur is None:
            continue
        s = line.strip()
        if m and line.startswith(".L"):
            if m.group(1).startswith(".Lfunc_end"):
                cur["closing"] = True
            else:
                pending.append(m.group(1))
            continue
        if cur.get("closing"):
            for key, pat in (("vgprs", r"; NumVgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"), ("occupancy", r"; Occupancy: (\d+)")):
                mm = re.match(pat, s)
                if mm:
                    cur["summary"][key] = int(mm.group(1))
            if "occupancy" in cur["summary"]:
                funcs[cur["name"]] = cur
                cur = None
            continue
        if s.startswith("; wave barrier"):
            cur["ins"].append(("wave_barrier", "", pending))
            pending = []
            continue
        if not s or s.startswith(";") or s.startswith("."):
            continue
        s = s.split(";")[0].strip()
        parts = s.split(None, 1)
        cur["ins"].append((parts[0], parts[1] if len(parts) > 1 else "", pending))
        pending = []
    return funcs


def is_load(op):
    return op.startswith(("global_load", "buffer_load", "flat_load", "scratch_load"))


def is_vmem(op):
    return op.startswith(("global_", "buffer_", "flat_", "scratch_"))


def is_sync(op):
    return op in ("s_barrier", "wave_barrier")


def is_valu(op):
    return op.startswith("v_")


def steady_loop(ins):
    """(first, last) instruction index of the largest natural loop: header label .. the furthest jump back to it."""
    where = {}
    for i, (_, _, labels) in enumerate(ins):
        for lab in labels:
            where[lab] = i
    best = None
    for i, (op, args, _) in enumerate(ins):
        if op.startswith(("s_cbranch", "s_branch")):
            tgt = where.get(args.strip())
            # (a jump back from a cold block laid out behind the kernel's end is no loop)
            if tgt is not None and tgt <= i and not any(o == "s_endpgm" for o, _, _ in ins[tgt:i]):
                # the loop's extent: blocks laid out behind the back edge may still belong to it (they jump back inside)
                end = i
                for j in range(i + 1, len(ins)):
                    o, a, _ = ins[j]
                    if o.startswith(("s_cbranch", "s_branch")) and tgt < where.get(a.strip(), -1) <= end:
                        end = j
                    if o == "s_endpgm":
                        break
                if best is None or end - tgt > best[1] - best[0]:
                    best = (tgt, end, i)
    return best, where


def fallthrough_path(ins, where, start, header, back, limit):
    """Instruction indices from `start` on along the fall-through path: conditional branches are not taken, except the
    loop's back edge; unconditional ones are followed."""
    i = start
    for _ in range(limit):
        yield i
        op, args, _ = ins[i]
        if op == "s_branch" or (i == back and op.startswith("s_cbranch")):
            i = where.get(args.strip(), i + 1)
        else:
            i += 1
        if i >= len(ins):
            return


def report_kernel(f):
    ins = f["ins"]
    rep = dict(f["summary"])
    loop, where = steady_loop(ins)
    if loop is None:
        rep["loop"] = None
        return rep
    head, end, back = loop
    # the main path of one step: header .. back edge, conditional branches not taken
    path = []
    for i in fallthrough_path(ins, where, head, head, -1, end - head + 1):
        if i > end or (path and i == head):
            break
        path.append(i)
        if ins[i][0] == "s_branch" and where.get(ins[i][1].strip()) == head:
            break
    pos = {i: k for k, i in enumerate(path)}
    loads = [i for i in path if is_load(ins[i][0])]
    syncs = [i for i in path if is_sync(ins[i][0])]
    lds_w = [i for i in path if ins[i][0].startswith("ds_write")]
    lds_r = [i for i in path if ins[i][0].startswith("ds_read")]
    body = [op for op, _, _ in ins[head:end + 1]]    # every block of the loop, whichever way its branches go
    rep["loop"] = {
        "instructions": len(path),
        "valu": sum(is_valu(ins[i][0]) for i in path),
        "all_blocks": {"instructions": len(body), "valu": sum(is_valu(op) for op in body), "s_nop": body.count("s_nop"),
                       "branches": sum(op.startswith(("s_cbranch", "s_branch")) for op in body)},
        "blocks_on_path": 1 + sum(bool(ins[i][2]) for i in path[1:]),
        "sync_kind": ("s_barrier" if any(ins[i][0] == "s_barrier" for i in syncs) else "wave fence") if syncs else None,
        "sync_at": [pos[i] for i in syncs],
        "load_at": [pos[i] for i in loads],
        "load_kinds": sorted({ins[i][0] for i in loads}),
        "first_lds_write_at": pos[lds_w[0]] if lds_w else None,
        "first_lds_read_at": pos[lds_r[0]] if lds_r else None,
    }
    lp = rep["loop"]
    if loads and syncs:
        first_sync = syncs[0]
        lp["loads_before_first_sync"] = all(pos[i] < pos[first_sync] for i in loads)
        # the first exchange's scatter ends with the last LDS write in front of that barrier / fence
        scat = [i for i in lds_w if pos[i] < pos[first_sync]]
        lp["first_scatter_ends_at"] = pos[scat[-1]] if scat else None
        lp["loads_behind_first_scatter"] = bool(scat) and all(pos[i] > pos[scat[-1]] for i in loads)
        # VALU instructions of one pass: between the first exchange's last sync and the second exchange's first
        per = 2 if len(syncs) % 2 == 0 and lp["sync_kind"] is not None and len(syncs) >= 4 else 1
        if len(syncs) >= per + 1:
            a, b = pos[syncs[per - 1]], pos[syncs[per]]
            lp["valu_one_pass"] = sum(is_valu(ins[i][0]) for i in path[a:b])
    if loads:
        # the wait that covers the last load: the first s_waitcnt vmcnt(k) behind it with k <= vector-memory
        # instructions issued since (vmcnt counts them in order)
        last = loads[-1]
        later, valu, lds, total, wait_at = 0, 0, 0, 0, None
        walk = fallthrough_path(ins, where, last, head, back, 2 * (end - head + 2))
        next(walk)
        for i in walk:
            op, args, _ = ins[i]
            if op == "s_waitcnt":
                m = _VMCNT.search(args)
                if m and int(m.group(1)) <= later:
                    wait_at = i
                    break
            if is_vmem(op):
                later += 1
            valu += is_valu(op)
            lds += op.startswith("ds_")
            total += 1
            if i < head or i > end:
                break
        lp["last_load_to_wait"] = {"valu": valu, "lds": lds, "instructions": total, "found": wait_at is not None,
                                   "wait": (ins[wait_at][0] + " " + ins[wait_at][1]) if wait_at is not None else None,
                                   "wait_at": pos.get(wait_at)}
    return rep


def kernel_key(name):
    m = re.search(r"welch_kernelILi(\d+)ELb([01])E", name)
    if m:
        return f"welch_kernel<{m.group(1)},{'true' if m.group(2) == '1' else 'false'}>"
    m = re.search(r"stream_scan_kernelILb([01])E", name)
    if m:
        return f"stream_scan_kernel<{'true' if m.group(1) == '1' else 'false'}>"
    return name


def report(text, name_re):
    funcs = split_functions(text, name_re)
    return {kernel_key(n): report_kernel(f) for n, f in funcs.items()}


def print_table(rep):
    for name, r in rep.items():
        print(f"{name}: {r.get('vgprs')} VGPRs, scratch {r.get('scratch')} B, occupancy {r.get('occupancy')}")
        lp = r.get("loop")
        if not lp:
            print("    no loop found")
            continue
        print(f"    steady-state loop: {lp['instructions']} instructions on the main path ({lp['valu']} VALU), "
              f"{lp['blocks_on_path']} block(s); exchanges ordered by {lp['sync_kind']} at {lp['sync_at']}")
        ab = lp["all_blocks"]
        print(f"    all blocks of the loop: {ab['instructions']} instructions, {ab['valu']} VALU, {ab['s_nop']} s_nop, {ab['branches']} branches")
        print(f"    first LDS write at {lp['first_lds_write_at']}, first LDS read at {lp['first_lds_read_at']}; "
              f"loads ({', '.join(lp['load_kinds']) or 'none'}) at {lp['load_at']}")
        if "loads_before_first_sync" in lp:
            print(f"    all loads in front of the first exchange's {lp['sync_kind']}: {lp['loads_before_first_sync']}; "
                  f"all behind its scatter (ends at {lp['first_scatter_ends_at']}): {lp['loads_behind_first_scatter']}; "
                  f"VALU in one pass: {lp.get('valu_one_pass')}")
        w = lp.get("last_load_to_wait")
        if w:
            print(f"    last load -> its wait ({w['wait']}, at {w['wait_at']}): {w['valu']} VALU, {w['lds']} LDS, "
                  f"{w['instructions']} instructions in all")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--source", default="k_welch.hip", help="file under gps-jamming_amd/csrc")
    ap.add_argument("--kernels", default="welch_kernel", help="regular expression a kernel's mangled name must contain")
    ap.add_argument("--asm", default=None, help="report on this assembly file instead of compiling")
    ap.add_argument("--keep-asm", default=None, help="write the assembly here")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if args.asm:
        text = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            path = args.keep_asm or os.path.join(tmp, "k.s")
            compile_to_asm(args.source, os.path.abspath(path))
            text = open(path).read()
    rep = report(text, args.kernels)
    if not rep:
        sys.exit(f"no kernel matching {args.kernels!r} in the assembly")
    if args.json:
        print(json.dumps(rep, indent=1))
    else:
        print_table(rep)


if __name__ == "__main__":
    main()
