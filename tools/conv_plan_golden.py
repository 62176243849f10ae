#!/usr/bin/env python3
"""Golden table of the conv dispatch plan (tests/golden/conv_plan.json).

Every entry is one host-only ``conv_plan(..., full=True)`` call: a conv shape and a named
request (REQUESTS: the pass — fwd, dgrad, wgrad — with its BN prologue, BN-statistics epilogue,
concatenated channels, requested splits / cfg, accumulate). "shapes" holds, per shape, the plan
of each request under the default knobs as the values of "fields"; "settings" holds, for every
other knob setting, only the fields that differ from the default ("<shape index>/<request>").
The dgrads are recorded with the BN-statistics epilogue: without it every plan is the same.
Requests in EDGE_ONLY are recorded for the small edge shapes only.

  python tools/conv_plan_golden.py --record     rewrite the table from the built extension
  python tools/conv_plan_golden.py --dump       plans of the table's rows under this process's
                                                environment, as JSON (tests/test_conv_plan.py
                                                runs this in a fresh child per env setting)

No GPU is needed: the plan is host arithmetic.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan.json")

# env settings that tests or recipes use; each needs a fresh process (read once at first use)
ENV_SETTINGS = ["SDX_CONV_CFG=4", "SDX_WGRAD3=0", "SDX_WGRAD1=0", "SDX_DGRAD_MERGE=0", "SDX_TAP_PAD=0",
                "SDX_CFG_RULES=7"]
# run-time setters, each on its own: (name, setter, argument tuple, tuple that restores the default)
SETTERS = [
    ("tap3_set(0)", "tap3_set", (0,), (1,)),
    ("wgrad_block_target_set(256)", "wgrad_block_target_set", (256,), (128,)),
    ("wgrad1x1_big_set(0)", "wgrad1x1_big_set", (0,), (1,)),
    ("wgrad1x1_big_set(2)", "wgrad1x1_big_set", (2,), (1,)),
    ("wgrad1x1_pairs_set(1)", "wgrad1x1_pairs_set", (1,), (0,)),
    ("igemm_one_k_set(0,64)", "igemm_one_k_set", (0, 64), (0, 256)),
    ("igemm_one_k_set(1,256)", "igemm_one_k_set", (1, 256), (1, 64)),
]


def _resnet_convs(name, N, size, stem):
    """(N, H, W, C, K, R, S, stride, pad) of every conv; input channels padded to 8."""
    convs = []
    if stem == "cifar":
        convs.append((N, size, size, 8, 64, 3, 3, 1, 1))
        h = size
    else:
        convs.append((N, size, size, 8, 64, 7, 7, 2, 3))
        h = size // 4   # 7x7/2 then 3x3/2 max-pool
    blocks = {"resnet18": [2, 2, 2, 2], "resnet50": [3, 4, 6, 3]}[name]
    bottleneck = name == "resnet50"
    exp = 4 if bottleneck else 1
    cin = 64
    for li, (planes, nb) in enumerate(zip([64, 128, 256, 512], blocks)):
        for b in range(nb):
            st = 2 if (li > 0 and b == 0) else 1
            ho = h // st
            if bottleneck:
                convs.append((N, h, h, cin, planes, 1, 1, 1, 0))
                convs.append((N, h, h, planes, planes, 3, 3, st, 1))
                convs.append((N, ho, ho, planes, planes * 4, 1, 1, 1, 0))
            else:
                convs.append((N, h, h, cin, planes, 3, 3, st, 1))
                convs.append((N, ho, ho, planes, planes, 3, 3, 1, 1))
            if st != 1 or cin != planes * exp:
                convs.append((N, h, h, cin, planes * exp, 1, 1, st, 0))
            cin, h = planes * exp, ho
    return convs


def shapes():
    out = []
    for N in (512, 256):
        for name in ("resnet18", "resnet50"):
            out += _resnet_convs(name, N, 32, "cifar")
    out += _resnet_convs("resnet50", 1024, 224, "imagenet")
    # the edge cases of the GPU tests: widths 4, 7, 8, 14, 28, 56; K or C = 64; a pixel count
    # not divisible by 32; stride-2 3x3 with Q outside {4, 8, 16, 32}
    for W in (4, 7, 8, 14, 28, 56):
        for C, K in ((64, 64), (128, 128), (64, 256), (256, 64)):
            out.append((2, W, W, C, K, 3, 3, 1, 1))
            out.append((2, W, W, C, K, 1, 1, 1, 0))
    for H in (14, 28, 56, 12, 20):          # Q = 7, 14, 28, 6, 10
        out.append((2, H, H, 64, 128, 3, 3, 2, 1))
        out.append((2, H, H, 128, 256, 1, 1, 2, 0))
    out += [(3, 5, 5, 128, 128, 1, 1, 1, 0), (3, 5, 5, 64, 64, 3, 3, 1, 1), (1, 9, 9, 128, 256, 1, 1, 1, 0),
            (5, 6, 6, 64, 128, 3, 3, 1, 1), (3, 10, 10, 128, 128, 3, 3, 2, 1), (1, 7, 7, 256, 128, 1, 1, 2, 0)]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


FIELDS = {
    "fwd": ["cfg", "mt", "nt", "depth", "one", "grid", "tap"],
    "dgrad": ["cfg", "mt", "nt", "depth", "one", "grid", "tap", "merged", "class_mt", "merged_mt"],
    "wgrad": ["family", "variant", "cfg", "steps", "per", "splits", "tiles", "slices", "slab_elems", "direct", "grid",
              "depth", "bn", "pairs", "slot"],
}
# request name -> [kind, in_bn, bnstat, cat_ch (-1: the conv's C), splits, cfg, accumulate]
REQUESTS = {
    "fwd": ["fwd", 0, 0, 0, 0, -1, 0],
    "fwd_bn": ["fwd", 1, 0, 0, 0, -1, 0],              # BN+ReLU operand prologue
    "dgrad": ["dgrad", 0, 1, 0, 0, -1, 0],
    "dgrad_cat": ["dgrad", 0, 1, -1, 0, -1, 0],        # K-concatenated conv3 dgrad (BN3 fold)
    "wgrad": ["wgrad", 0, 0, 0, 0, -1, 1],             # as the training step: into the gradient sink
    "wgrad_new": ["wgrad", 0, 0, 0, 0, -1, 0],
    "wgrad_generic": ["wgrad", 0, 0, 0, 0, -2, 0],
    "wgrad_splits3": ["wgrad", 0, 0, 0, 3, -1, 0],
    "wgrad_bn": ["wgrad", 1, 0, 0, 0, -1, 1],          # BN+ReLU operand prologue
}
EDGE_ONLY = {"fwd_bn", "wgrad_new", "wgrad_generic", "wgrad_splits3", "wgrad_bn"}   # shapes with N <= 5


def requests_of(shape):
    N, H, W, C, K, R, S, st, pad = shape
    out = []
    for name in REQUESTS:
        if name in EDGE_ONLY and N > 5:
            continue
        if name == "dgrad_cat" and not (R == 1 and st == 1 and K == 4 * C):
            continue
        out.append(name)
    return out


def compute(m, shape, name):
    """The plan of one (shape, request) as the list of FIELDS values."""
    N, H, W, C, K, R, S, st, pad = shape
    kind, in_bn, bnstat, cat_ch, splits, cfg, acc = REQUESTS[name]
    d = m.conv_plan(N, H, W, C, K, R, S, st, pad, kind == "dgrad", full=True, kind=kind, in_bn=bool(in_bn),
                    bnstat=bool(bnstat), cat_ch=C if cat_ch < 0 else cat_ch, splits=splits, cfg=cfg,
                    accumulate=bool(acc))
    assert d["ok"]
    return [d[f] for f in FIELDS[kind]]


def compute_all(m, shape_list):
    return {f"{i}/{n}": compute(m, s, n) for i, s in enumerate(shape_list) for n in requests_of(s)}


def changed(base, rows):
    """{entry: {field: value}} of the fields that differ from the default plan."""
    out = {}
    for key, row in rows.items():
        fields = FIELDS[REQUESTS[key.split("/")[1]][0]]
        ch = {f: v for f, v, b in zip(fields, row, base[key]) if v != b}
        if ch:
            out[key] = ch
    return out


def _ext():
    sys.path.insert(0, ROOT)
    from simclr_pytorch_distributed_amd.ops import _ext as e
    m = e.ext()
    if m is None:
        raise SystemExit("native extension not built (python csrc/build.py)")
    return m


def child_dump(setting, shape_list):
    env = dict(os.environ)
    name, val = setting.split("=")
    env[name] = val
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump"], env=env, input=json.dumps(shape_list),
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    return json.loads(r.stdout)


def record():
    m = _ext()
    sl = [list(s) for s in shapes()]
    base = compute_all(m, sl)
    settings = {}
    for name, setter, args, restore in SETTERS:
        getattr(m, setter)(*args)
        try:
            settings[name] = changed(base, compute_all(m, sl))
        finally:
            getattr(m, setter)(*restore)
    assert compute_all(m, sl) == base, "a setter was not restored"
    for s in ENV_SETTINGS:
        settings[s] = changed(base, child_dump(s, sl))
    c = lambda x: json.dumps(x, separators=(",", ":"))   # noqa: E731
    with open(GOLDEN, "w") as f:
        f.write('{"fields": ' + json.dumps(FIELDS) + ',\n"requests": ' + json.dumps(REQUESTS) + ',\n"shapes": [\n')
        f.write(",\n".join(c([s, {n: base[f"{i}/{n}"] for n in requests_of(s)}]) for i, s in enumerate(sl)))
        f.write('\n],\n"settings": {\n')
        f.write(",\n".join(json.dumps(n) + ": {\n" + ",\n".join(f'"{k}":{c(v)}' for k, v in o.items()) + "}"
                           for n, o in settings.items()))
        f.write("\n}}\n")
    print(f"{len(sl)} shapes, {len(base)} plans, " + ", ".join(f"{n}: {len(o)} differ" for n, o in settings.items()))
    print(f"{os.path.getsize(GOLDEN)} bytes -> {GOLDEN}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--dump", action="store_true", help="plans of the shape list read as JSON from stdin")
    a = ap.parse_args()
    if a.record:
        record()
    elif a.dump:
        json.dump(compute_all(_ext(), json.load(sys.stdin)), sys.stdout, separators=(",", ":"))
    else:
        ap.print_help()


if __name__ == "__main__":
    main()
