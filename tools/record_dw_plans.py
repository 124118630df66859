#!/usr/bin/env python
"""Records what the weight-gradient (dW) host path of cape_amd/csrc/gconv.hip DECIDES, without a GPU: pure ctypes over placeholder
addresses that are never dereferenced (as tests/test_dw_batch_plan.py and tests/h2_cases.py do).

    python tools/record_dw_plans.py            writes tests/dw_plan_table.json
    python tools/record_dw_plans.py --digest   prints the sha256 of the whole grid's rows (one process = one setting of the CAPE_*
                                               switches: the library latches them at first use)

tests/test_dw_plan_table.py recomputes everything and compares it with the committed table, so a change of the host code that
moves a kernel choice, a tile, a slab count, a workspace size, a batch plan or a return code fails on the CPU.

The grid (every combination):
    storage      fp32, bf16
    row bounds   fp32 only: none (cape_gconv_dw_plan), or on every operand (cape_gconv_dw_plan_h2); bf16: cape_gconv_dw_plan_bf16
    dz2          absent, or masked onto the last source
    base         every operand 16-byte aligned, or 4 bytes off
    sources      SOURCES below (channels, row pitch)
    F            FS below with lddz = round_up(F, 4); the F that are no multiple of 4 also with lddz = F
    (N, Mo)      SHAPES below
A row is (storage, bounds, dz2, off, source list, F, lddz, N, Mo | rc, plan[0..3], workspace bytes, and for the cases with row
bounds the return code of cape_gconv_dw_batch_plan on the case alone: 0 where the batched contraction takes it).

The table holds the full rows of a readable subset (about 200: the first case of every (storage, kernel id, ct, ft) the grid
reaches, then every n-th case), one sha256 over all rows, the same digest under each of five switches set to 0, the plans of
cape_gconv_dw_batch_plan for the lists of tests/test_dw_batch_plan.py, and the return codes of the argument errors."""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TABLE = os.path.join(ROOT, "tests", "dw_plan_table.json")
SOURCES = [[(3, 4)], [(3, 3)], [(5, 5)], [(16, 16)], [(32, 32)] * 2, [(32, 32)] * 3, [(48, 48)], [(64, 64)], [(64, 64)] * 2,
           [(128, 128)], [(128, 128)] * 3, [(160, 160)], [(256, 256)] * 2, [(512, 512)] * 2]
FS = [1, 3, 4, 10, 16, 32, 64, 66, 128, 192, 256, 512]
SHAPES = [(1, 70), (2, 431), (3, 1723), (16, 862), (16, 6890)]
SWITCHES = ["CAPE_DW_PLAIN", "CAPE_DW_BF16X6", "CAPE_DW_H2", "CAPE_DW_V4", "CAPE_NARROW"]
# knobs that move a dW plan: the default digest and the subset are taken with none of them set
PLAN_KNOBS = SWITCHES + ["CAPE_H2"]
SUBSET = 200

# Kernel ids (plan[0]): 0 generic, 1 plain, 2 packed, 3 split, 4 h2, 5 narrow-in, 6 narrow-out.  The (ct, ft) each id reports on
# this grid, from the rules of gconv.hip (written down here, not read off the library):
#   * ids 0, 3, 4 plan with plan_dw: ct = 64 for sources of at most 64 channels else 128, ft = 64 for F <= 64 else 128; the
#     grid has sources and F on both sides of 64 for each of them
#   * id 1 (fp32) is what stays plain but neither packs, nor splits (channels no multiple of 4, or F odd), nor is narrow: the
#     3- and 5-channel sources (ct 64) at any F, and wider sources at F = 1, 3 with dz2 in play (ft 64); (128, 128) needs an odd
#     F above 64 or a wide source with channels no multiple of 4, which the grid does not have
#   * id 1 (bf16, no narrow forms) also takes 4-channel-multiple sources at odd F: the same three tiles
#   * id 2 plans with plan_dw_plain and needs F <= 64 and at most 128 channels in all: ft = 32 (always with ct 128) or 64;
#     [32, 32] gives (128, 32) and (64, 64), [32, 32, 32] gives (128, 32) and (128, 64)
#     (bf16 splits before it packs, so only F = 1, 3 pack there: ft 32)
#   * id 5 (fp32): at most 8 channels in all, 16 <= F <= 256 in multiples of 4: the (3, ld 4) source, ct 64, both ft
#   * id 6 (fp32): F <= 4 and 16..256 channels in multiples of 4: both ct, ft 64; it reports the tiles of the family it
#     replaces, and several sources of at most 128 channels in all would have packed: (128, 32) as well
_SQUARE = {(64, 64), (64, 128), (128, 64), (128, 128)}
EXPECT_TILES = {
    ("fp32", 0): _SQUARE, ("fp32", 1): {(64, 64), (64, 128), (128, 64)}, ("fp32", 2): {(128, 32), (64, 64), (128, 64)},
    ("fp32", 3): _SQUARE, ("fp32", 4): _SQUARE, ("fp32", 5): {(64, 64), (64, 128)}, ("fp32", 6): {(64, 64), (128, 64), (128, 32)},
    ("bf16", 0): _SQUARE, ("bf16", 1): {(64, 64), (64, 128), (128, 64)}, ("bf16", 2): {(128, 32)},
    ("bf16", 3): _SQUARE,
}


def _load():
    from cape_amd import _lib
    return _lib, _lib.lib


def make_case(_lib, storage, bounds, two, off, srcl, F, lddz, N, Mo):
    """(srcs array, dz, dz sample stride, dz2, mask, h2 or None, keep-alive) over made-up addresses."""
    es = 2 if storage == "bf16" else 4
    assert off % es == 0
    srcs = (_lib.CapeSrc * len(srcl))()
    h2 = _lib.CapeH2Dw() if bounds else None
    base = 0x10000000
    for i, (s, (Cn, ld)) in enumerate(zip(srcs, srcl)):
        base += 0x4000000
        s.x, s.x_sample_stride, s.ldx, s.C = base + off, Mo * ld, ld, Cn
        s.w, s.w_rs, s.w_cs = base + 0x2000000, F, 1
        s.w2, s.w2_rs, s.w2_cs = None, 0, 0
        if bounds:
            h2.src_rowmax[i], h2.src_rowmax_w[i] = base + 0x3000000, 4 * -(-Cn // 128)
    base += 0x4000000
    dz, dz2, mask = base + off, None, 0
    if bounds:
        h2.dz_rowmax, h2.dz_rowmax_w = base + 0x3000000, 4 * -(-F // 128)
    if two:
        dz2, mask = base + 0x1000000 + off, 1 << (len(srcl) - 1)
        if bounds:
            h2.dz2_rowmax, h2.dz2_rowmax_w = base + 0x3800000, 4 * -(-F // 128)
    return srcs, dz, Mo * lddz, dz2, mask, h2, (srcs, h2)


def plan_of(lib, storage, srcs, n, dz, dzs, lddz, dz2, mask, N, Mo, F, h2):
    plan = (C.c_int32 * 4)(-9, -9, -9, -9)
    if storage == "bf16":
        rc = lib.cape_gconv_dw_plan_bf16(srcs, n, dz, dzs, lddz, dz2, mask, N, Mo, F, plan)
    elif h2 is not None:
        rc = lib.cape_gconv_dw_plan_h2(srcs, n, dz, dzs, lddz, dz2, mask, N, Mo, F, C.byref(h2), plan)
    else:
        rc = lib.cape_gconv_dw_plan(srcs, n, dz, dzs, lddz, dz2, mask, N, Mo, F, plan)
    return rc, list(plan)


def grid():
    for storage in ("fp32", "bf16"):
        for bounds in ((0, 1) if storage == "fp32" else (0,)):
            for two in (0, 1):
                for off in (0, 4):
                    for srcl in SOURCES:
                        for F in FS:
                            for lddz in sorted({(F + 3) & ~3, F}, reverse=True):
                                for N, Mo in SHAPES:
                                    yield storage, bounds, two, off, srcl, F, lddz, N, Mo


def grid_rows():
    _lib, lib = _load()
    rows = []
    for case in grid():
        storage, bounds, two, off, srcl, F, lddz, N, Mo = case
        srcs, dz, dzs, dz2, mask, h2, keep = make_case(_lib, *case)
        rc, plan = plan_of(lib, storage, srcs, len(srcl), dz, dzs, lddz, dz2, mask, N, Mo, F, h2)
        wsb = lib.cape_gconv_dw_workspace_bytes(srcs, len(srcl), N, Mo, F)
        joins = None
        if h2 is not None:                 # would the batched contraction take it (dw_h2_kernel<128, 128, true>)?  0 = yes
            it = (_lib.CapeDwItem * 1)()
            it[0].srcs, it[0].nsrc, it[0].dz, it[0].dz_sample_stride, it[0].lddz = C.addressof(srcs), len(srcl), dz, dzs, lddz
            it[0].dz2, it[0].dz2_mask, it[0].N, it[0].Mo, it[0].F = dz2, mask, N, Mo, F
            it[0].workspace, it[0].workspace_bytes, it[0].h2 = 0x70000000, wsb, C.addressof(h2)
            joins = lib.cape_gconv_dw_batch_plan(C.addressof(it), 1, None, 0, (C.c_int32 * 4)())
        rows.append([storage, bounds, two, off, [list(s) for s in srcl], F, lddz, N, Mo, rc] + plan + [int(wsb), joins])
    return rows


def digest(rows):
    h = hashlib.sha256()
    for r in rows:
        h.update((json.dumps(r, separators=(",", ":")) + "\n").encode())
    return h.hexdigest()


def subset_of(rows):
    """Asserts the coverage of the grid, then picks the readable subset: first case of every (storage, id, ct, ft), then a stride."""
    seen, first = {}, []
    for i, r in enumerate(rows):
        assert r[9] == 0, r
        key = (r[0], r[10], r[11], r[12])
        if key not in seen:
            seen[key] = i
            first.append(i)
    got = {}
    for storage, kid, ct, ft in seen:
        got.setdefault((storage, kid), set()).add((ct, ft))
    assert sorted(got) == sorted(EXPECT_TILES), sorted(got)
    for k, tiles in EXPECT_TILES.items():
        assert got[k] == tiles, (k, sorted(got[k]), sorted(tiles))
    step = len(rows) // (SUBSET - len(first))
    picked = sorted(set(first) | set(range(step // 2, len(rows), step)))
    sub = [rows[i] for i in picked]
    assert {(r[0], r[10], r[11], r[12]) for r in sub} == set(seen)
    return sub


def batch_lists():
    """The lists of tests/test_dw_batch_plan.py: both phases of the benchmarked step, and its six seeded random lists."""
    import test_dw_batch_plan as T
    out = [("decoder", T.DECODER, 16), ("encoder", T.ENCODER, 16)]
    for seed in range(6):
        rng = random.Random(seed)
        N = rng.choice([1, 2, 3, 6, 12, 16])
        shapes = []
        for _ in range(rng.randint(1, 12)):
            nsrc = rng.randint(1, 4)
            Cn = rng.choice([128, 160, 256, 384, 512])
            F = rng.choice([128, 192, 256, 512])
            Mo = rng.choice([431, 862, 1000, 1723, 3445])
            two = rng.randrange(nsrc) if rng.random() < 0.3 else None
            shapes.append(([Cn] * nsrc, Mo, F, two))
        out.append(("random%d" % seed, shapes, N))
    return out


def batch_plans():
    import test_dw_batch_plan as T
    out = {}
    for name, shapes, N in batch_lists():
        arr, keep, facts = T.make_items(shapes, N)
        rows, info = T.query(arr, len(shapes))
        out[name] = dict(info=info, units_sha256=digest([list(r) for r in rows]))
    return out


def error_cases():
    """name -> [rc of cape_gconv_dw_plan, rc of cape_gconv_dw_stage (null stream)].  Every one of them returns before any launch:
    the stage entry validates its arguments, then the workspace size, then the sources, and only then launches."""
    _lib, lib = _load()
    F, N, Mo = 64, 2, 70
    big = 1 << 40

    def run(srcl=((64, 64),), nsrc=None, lddz=64, mask=0, two=False, stage=0, ws=0x70000000, wsb=big, null_srcs=False,
            null_w=False, ldx=None, null_plan=False):
        srcs, dz, dzs, dz2, m, h2, keep = make_case(_lib, "fp32", 0, 0, 0, list(srcl), F, lddz, N, Mo)
        if two:
            dz2 = dz + 0x1000000
        if null_w:
            srcs[0].w = None
        if ldx is not None:
            srcs[0].ldx = ldx
        n = len(srcl) if nsrc is None else nsrc
        a = None if null_srcs else srcs
        plan = (C.c_int32 * 4)()
        rc_plan = lib.cape_gconv_dw_plan(a, n, dz, dzs, lddz, dz2, mask, N, Mo, F, None if null_plan else plan)
        rc_stage = lib.cape_gconv_dw_stage(a, n, dz, dzs, lddz, dz2, mask, N, Mo, F, 0, ws, wsb, stage, None)
        return [rc_plan, rc_stage]

    srcs, dz, dzs, dz2, m, h2, keep = make_case(_lib, "fp32", 0, 0, 0, [(64, 64)], F, 64, N, Mo)
    rc, plan = plan_of(lib, "fp32", srcs, 1, dz, dzs, 64, None, 0, N, Mo, F, None)
    assert rc == 0
    need = 64 * F * plan[3] * 4                      # the partial slabs of this launch
    return {
        "null_srcs": run(null_srcs=True),
        "nsrc_0": run(nsrc=0),
        "nsrc_9": run(nsrc=9),
        "lddz_below_F": run(lddz=63),
        "dz2_mask_without_dz2": run(mask=1),
        "stage_3": run(stage=3),
        "stage_negative": run(stage=-1),
        "null_workspace": run(ws=None),
        "workspace_one_byte_short": run(wsb=need - 1),
        "workspace_short_and_null_weight": run(wsb=0, null_w=True),
        "null_weight_block": run(null_w=True),
        "source_pitch_below_channels": run(ldx=60),
    }


def switch_digest(name):
    env = {k: v for k, v in os.environ.items() if k not in PLAN_KNOBS}
    if name:
        env[name] = "0"
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--digest"], env=env, check=True, stdout=subprocess.PIPE,
                         universal_newlines=True).stdout
    return out.strip().splitlines()[-1]


def main():
    if "--digest" in sys.argv[1:]:
        print(digest(grid_rows()))
        return
    if any(k in os.environ for k in PLAN_KNOBS):
        sys.exit("unset %s first: the table is recorded with the library's defaults" % ", ".join(PLAN_KNOBS))
    rows = grid_rows()
    table = dict(
        columns=["storage", "bounds", "dz2", "off", "sources (C, ld)", "F", "lddz", "N", "Mo", "rc", "kernel", "ct", "ft", "slabs",
                 "workspace_bytes", "batch_plan_rc"],
        grid_cases=len(rows), grid_sha256=digest(rows), subset=subset_of(rows),
        switch_sha256={k: switch_digest(k) for k in SWITCHES},
        batch_plans=batch_plans(), errors=error_cases())
    with open(TABLE, "w") as f:
        f.write("{\n")
        keys = list(table)
        for k in keys:
            end = ",\n" if k != keys[-1] else "\n"
            if k == "subset":
                f.write(' "subset": [\n' + ",\n".join("  " + json.dumps(r) for r in table[k]) + "\n ]" + end)
            else:
                f.write(" %s: %s%s" % (json.dumps(k), json.dumps(table[k], sort_keys=True), end))
        f.write("}\n")
    print("%d grid cases, %d in the subset -> %s" % (len(rows), len(table["subset"]), TABLE))


if __name__ == "__main__":
    main()
