#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 code of every ``csrc/kernels/*.hip`` unit (host-only).

Each unit is compiled to assembly (device side only) with the flags ``csrc/build.py`` gives
it, and every kernel gets one line::

    <demangled name> \t vgpr= agpr= sgpr= lds= scratch= \t <sha1> \t <unit>

The sha1 covers the kernel's whole text (label to function end, its ``.amdhsa_kernel``
block included) after comments are dropped, local labels are renumbered by first appearance
and references to the per-unit device globals (the zero pages, the igemm trace buffer) are
folded to fixed tokens, so a kernel that moves to another unit unchanged keeps its digest.
``# unit`` lines give each unit's compile time (units compile ``--jobs`` at a time; use
``--jobs 1`` for serial times).

    python tools/isa_digest.py [--jobs N] [--define NAME=V] [--checked] > after.txt
    python tools/isa_digest.py --diff before.txt after.txt

``--diff`` lists kernels missing, added, or changed in digest or resources (exit status 1
if any); a kernel that only changed unit is not a difference.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
import time
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "csrc"))
import build as sdx_build  # noqa: E402

_LOCAL = re.compile(r"\.L[A-Za-z0-9_$.]+")
# per-unit device globals (anonymous namespace, one copy per including unit)
_GLOBALS = ((re.compile(r"\b\w*(?:g_zero16|w1_zero16|w3_zero16)\w*"), "$zero16"),
            (re.compile(r"\b\w*g_igemm_trace\w*"), "$igemm_trace"))
_RES = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("accum", "accum_offset"),
        ("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size"))


def _normalise(lines):
    labels = {}
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].strip()
        if not ln:
            continue
        for rx, tok in _GLOBALS:
            ln = rx.sub(tok, ln)
        ln = _LOCAL.sub(lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), ln)
        out.append(ln)
    return "\n".join(out)


def kernels_of(asm_text):
    """[(mangled name, resources dict, sha1)] of one unit's assembly, in file order."""
    lines = asm_text.splitlines()
    start = {}
    for i, ln in enumerate(lines):
        if ln and not ln[0].isspace() and not ln.startswith(".L"):
            start.setdefault(ln.split(":", 1)[0], i)
    out = []
    for i, ln in enumerate(lines):
        s = ln.strip()
        if not s.startswith(".amdhsa_kernel "):
            continue
        name = s.split()[1]
        res = {}
        j = i
        while not lines[j].strip().startswith(".end_amdhsa_kernel"):
            f = lines[j].split()
            for key, directive in _RES:
                if f and f[0] == ".amdhsa_" + directive:
                    res[key] = int(f[1])
            j += 1
        while not lines[j].startswith(".Lfunc_end"):
            j += 1
        res["agpr"] = res["vgpr"] - min(res["vgpr"], res.pop("accum"))
        text = _normalise(lines[start[name] + 1:j])
        out.append((name, res, hashlib.sha1(text.encode()).hexdigest()))
    return out


def _demangle(names):
    if not names:
        return []
    r = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    return r.stdout.splitlines()


def digest(jobs, checked, defines, keep):
    kdir = os.path.join(ROOT, "csrc", "kernels")
    units = sorted(f for f in os.listdir(kdir) if f.endswith(".hip"))
    tmp = keep or tempfile.mkdtemp(prefix="isa_digest_")
    os.makedirs(tmp, exist_ok=True)

    def one(unit):
        src = os.path.join(kdir, unit)
        asm = os.path.join(tmp, unit[:-4] + ".s")
        cmd = sdx_build.kernel_flags(src, checked=checked, defines=defines) + ["--cuda-device-only", "-S", src, "-o", asm]
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True)
        dt = time.time() - t0
        if r.returncode != 0:
            raise RuntimeError(f"compile failed: {unit}\n{r.stderr}")
        with open(asm) as fh:
            text = fh.read()
        return unit, dt, text.count("\n"), kernels_of(text)

    t0 = time.time()
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        results = list(ex.map(one, units))
    wall = time.time() - t0
    for unit, dt, nlines, ks in results:
        print(f"# unit {unit}\tcompile_s={dt:.1f}\tkernels={len(ks)}\tasm_lines={nlines}")
    print(f"# total\twall_s={wall:.1f}\tjobs={jobs}\tkernels={sum(len(r[3]) for r in results)}")
    rows = []
    for unit, _, _, ks in results:
        for (_, res, sha), dem in zip(ks, _demangle([k[0] for k in ks])):
            rs = " ".join(f"{k}={res[k]}" for k in ("vgpr", "agpr", "sgpr", "lds", "scratch"))
            rows.append(f"{dem}\t{rs}\t{sha}\t{unit}")
    print("\n".join(sorted(rows)))
    if not keep:
        for f in os.listdir(tmp):
            os.unlink(os.path.join(tmp, f))
        os.rmdir(tmp)


def _load(path):
    rows = {}
    seen = Counter()
    with open(path) as fh:
        for ln in fh:
            if ln.startswith("#") or not ln.strip():
                continue
            name, res, sha, unit = ln.rstrip("\n").split("\t")
            seen[name] += 1   # the same internal-linkage kernel instantiated by two units
            rows[(name, seen[name])] = (res, sha, unit)
    return rows


def diff(a_path, b_path):
    a, b = _load(a_path), _load(b_path)
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in b:
            print(f"missing\t{k[0]}\t(was in {a[k][2]})")
        elif k not in a:
            print(f"added\t{k[0]}\t(in {b[k][2]})")
        elif a[k][:2] != b[k][:2]:
            what = "resources" if a[k][0] != b[k][0] else "digest"
            print(f"changed {what}\t{k[0]}\t{a[k][0]} {a[k][1][:10]} ({a[k][2]}) -> {b[k][0]} {b[k][1][:10]} ({b[k][2]})")
        else:
            continue
        bad += 1
    moved = sum(1 for k in a if k in b and a[k][2] != b[k][2])
    print(f"# {len(a)} kernels before, {len(b)} after: {bad} missing / added / changed, {moved} in another unit")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 4))
    ap.add_argument("--checked", action="store_true", help="digest the --checked build's kernels")
    ap.add_argument("--define", action="append", default=[], help="extra kernel define NAME=VALUE")
    ap.add_argument("--keep", default="", help="keep the .s files in this directory")
    a = ap.parse_args()
    if a.diff:
        return diff(*a.diff)
    digest(a.jobs, a.checked, a.define, a.keep)
    return 0


if __name__ == "__main__":
    sys.exit(main())
