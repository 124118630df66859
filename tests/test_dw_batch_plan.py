"""cape_gconv_dw_batch_plan (pure host logic, no GPU): the plan of the batched weight-gradient contraction -- the queued launches of
dw_h2_kernel<128, 128, true> of one backward phase as one grid.  Checked on the nine such launches of the benchmarked step (CAPE-
affineconv nz64, batch 16: four in the decoder's phase, five in the encoder's) and on seeded random lists: every (item, tile, row)
is contracted exactly once, by workgroups with contiguous row ranges; an item is cut into exactly the splits of its own launch
(its workspace holds those slabs, its reduction counts them, and the results stay bit for bit what they were); all tiles of a split
share an XCD; the kernel arguments fit 4 KB, a longer list is cut into several launches; the plan is a function of its input."""
import ctypes as C
import random

import pytest

from cape_amd import _lib

lib = _lib.lib

# (sources' channels, vertices, output channels, source index that contracts against dz2 or None)
DECODER = [([128, 128, 128], 1723, 128, 2), ([128, 128, 128], 862, 256, None), ([256, 256, 256], 862, 256, 2),
           ([512, 512, 512], 862, 256, 2)]
ENCODER = [([512, 512], 862, 512, None), ([256, 256], 862, 512, None), ([256, 256], 862, 256, None), ([128, 128], 1723, 256, None),
           ([128, 128], 1723, 128, None)]


def make_items(shapes, N=16):
    """cape_dw_item_t array over made-up (never dereferenced) addresses; returns (array, keep-alive, per-item facts)."""
    arr = (_lib.CapeDwItem * len(shapes))()
    keep, facts = [], []
    base = 0x10000000
    for it, (Cs, Mo, F, two) in zip(arr, shapes):
        srcs = (_lib.CapeSrc * len(Cs))()
        h2 = _lib.CapeH2Dw()
        for i, (s, Cn) in enumerate(zip(srcs, Cs)):
            base += 0x1000000
            s.x, s.x_sample_stride, s.ldx, s.C = base, Mo * Cn, Cn, Cn
            s.w, s.w_rs, s.w_cs = base + 0x800000, F, 1
            s.w2, s.w2_rs, s.w2_cs = None, 0, 0
            h2.src_rowmax[i], h2.src_rowmax_w[i] = base + 0x400000, 4 * -(-Cn // 128)
        base += 0x1000000
        h2.dz_rowmax, h2.dz_rowmax_w = base + 0x400000, 4 * -(-F // 128)
        it.srcs, it.nsrc = C.addressof(srcs), len(Cs)
        it.dz, it.dz_sample_stride, it.lddz = base, Mo * F, F
        it.dz2, it.dz2_mask = None, 0
        if two is not None:
            it.dz2, it.dz2_mask = base + 0x800000, 1 << two
            h2.dz2_rowmax, h2.dz2_rowmax_w = base + 0xC00000, 4 * -(-F // 128)
        it.N, it.Mo, it.F, it.accumulate, it.bf16 = N, Mo, F, 0, 0
        it.workspace_bytes = lib.cape_gconv_dw_workspace_bytes(srcs, len(Cs), N, Mo, F)
        base += 0x1000000
        it.workspace = base
        it.h2 = C.addressof(h2)
        keep += [srcs, h2]
        own = (C.c_int32 * 4)()
        assert lib.cape_gconv_dw_plan_h2(srcs, len(Cs), it.dz, it.dz_sample_stride, it.lddz, it.dz2, it.dz2_mask, N, Mo, F, C.byref(h2), own) == 0
        facts.append(dict(Cs=Cs, Mo=Mo, F=F, N=N, own=list(own)))
    return arr, keep, facts


def query(arr, n):
    info = (C.c_int32 * 4)()
    assert lib.cape_gconv_dw_batch_plan(C.addressof(arr), n, None, 0, info) == 0
    units = (C.c_int32 * (10 * max(1, info[1])))()
    info2 = (C.c_int32 * 4)()
    assert lib.cape_gconv_dw_batch_plan(C.addressof(arr), n, units, info[1], info2) == 0
    assert list(info) == list(info2)
    rows = [tuple(units[10 * u:10 * u + 10]) for u in range(info[1])]
    return rows, list(info)


def check_plan(shapes, N=16):
    arr, keep, facts = make_items(shapes, N)
    n = len(shapes)
    rows, info = query(arr, n)
    nlaunch, nunits, arg_bytes, grid = info
    assert arg_bytes <= 4096 and nlaunch >= 1 and nunits == len(rows)
    # the same input gives the same plan
    assert query(arr, n) == (rows, info)
    # every launch's blocks are distinct and inside the grid
    per_launch = {}
    for r in rows:
        per_launch.setdefault(r[0], []).append(r)
    assert sorted(per_launch) == list(range(nlaunch))
    for l, rs in per_launch.items():
        blocks = [r[1] for r in rs]
        assert len(set(blocks)) == len(blocks) and 0 <= min(blocks) and max(blocks) < grid
        # all tiles of one (item, slab) run on one XCD (block & 7): they read the same operand rows
        xcd = {}
        for r in rs:
            assert xcd.setdefault((r[2], r[5]), r[1] & 7) == r[1] & 7
        # an XCD runs its longest workgroups first (an item's length: samples x rows of its first row range)
        plen = {}
        for r in rs:
            if r[8] == 0:
                plen[r[2]] = (r[7] - r[6]) * (-(-(r[9] - r[8]) // 32) * 32)      # (whole 32-row chunks)
        for x in range(8):
            seq = [plen[r[2]] for r in sorted((r for r in rs if r[1] & 7 == x), key=lambda r: r[1])]
            assert seq == sorted(seq, reverse=True), (l, x, seq)
    # launches take the items in list order, each item in exactly one; no launch beyond what the argument table holds
    launch_of = [sorted(set(r[0] for r in rows if r[2] == i)) for i in range(n)]
    assert all(len(x) == 1 for x in launch_of) and [x[0] for x in launch_of] == sorted(x[0] for x in launch_of)
    for l in range(nlaunch):
        members = [i for i in range(n) if launch_of[i][0] == l]
        assert len(members) <= 6 and sum(len(facts[i]["Cs"]) for i in members) <= 12
    for i, f in enumerate(facts):
        fam, ct, ft, own_slabs = f["own"]
        assert (fam, ct, ft) == (4, 128, 128)
        mine = [u for u in rows if u[2] == i]
        # the slabs of the item's own launch, 0 .. own_slabs - 1, each with every tile of every source exactly once
        want_tiles = sorted((s, t) for s, c in enumerate(f["Cs"]) for t in range(-(-c // 128) * -(-f["F"] // 128)))
        by_slab = {}
        for u in mine:
            by_slab.setdefault(u[5], []).append(u)
        assert sorted(by_slab) == list(range(own_slabs))
        cover = {}
        for slab, us in by_slab.items():
            assert sorted((u[3], u[4]) for u in us) == want_tiles
            ranges = set(u[6:10] for u in us)
            assert len(ranges) == 1                              # one (sample range, row range) per slab
            n0, n1, r0, r1 = ranges.pop()
            assert 0 <= n0 < n1 <= f["N"] and 0 <= r0 < r1 <= f["Mo"] and r0 % 32 == 0
            for smp in range(n0, n1):
                cover.setdefault(smp, []).append((r0, r1))
        # every sample's rows 0 .. Mo: contiguous ranges, no gap, no overlap
        assert sorted(cover) == list(range(f["N"]))
        for smp, rr in cover.items():
            rr.sort()
            assert rr[0][0] == 0 and rr[-1][1] == f["Mo"] and all(a[1] == b[0] for a, b in zip(rr, rr[1:]))
    return rows, info


@pytest.mark.parametrize("phase", ["decoder", "encoder"])
def test_phases_of_the_benchmarked_step(phase):
    shapes = DECODER if phase == "decoder" else ENCODER
    rows, info = check_plan(shapes)
    assert info[0] == 1                                          # one launch per phase
    # the 8 XCDs get equal shares of the workgroups (every split count of the step is a multiple of 8)
    per = [sum(1 for u in rows if u[1] & 7 == x) for x in range(8)]
    assert max(per) == min(per), per


def test_single_item_and_argument_errors():
    check_plan([ENCODER[0]])
    arr, keep, facts = make_items([ENCODER[0]])
    info = (C.c_int32 * 4)()
    assert lib.cape_gconv_dw_batch_plan(None, 1, None, 0, info) == -1
    assert lib.cape_gconv_dw_batch_plan(C.addressof(arr), 0, None, 0, info) == -1
    assert lib.cape_gconv_dw_batch_plan(C.addressof(arr), 13, None, 0, info) == -1
    # a launch that does not run dw_h2_kernel<128, 128, true> cannot join: 64-channel sources (64 x 128 tiles), missing row bounds
    arr, keep, facts = make_items([([128, 128], 862, 256, None)])
    arr[0].h2 = None
    assert lib.cape_gconv_dw_batch_plan(C.addressof(arr), 1, None, 0, info) == -1
    a64 = (_lib.CapeDwItem * 1)()
    srcs = (_lib.CapeSrc * 1)()
    h2 = _lib.CapeH2Dw()
    srcs[0].x, srcs[0].x_sample_stride, srcs[0].ldx, srcs[0].C = 0x10000000, 3445 * 64, 64, 64
    srcs[0].w, srcs[0].w_rs, srcs[0].w_cs = 0x20000000, 128, 1
    h2.src_rowmax[0], h2.src_rowmax_w[0], h2.dz_rowmax, h2.dz_rowmax_w = 0x30000000, 4, 0x40000000, 4
    a64[0].srcs, a64[0].nsrc, a64[0].dz, a64[0].dz_sample_stride, a64[0].lddz = C.addressof(srcs), 1, 0x50000000, 3445 * 128, 128
    a64[0].N, a64[0].Mo, a64[0].F, a64[0].workspace, a64[0].workspace_bytes, a64[0].h2 = 16, 3445, 128, 0x60000000, 1 << 40, C.addressof(h2)
    assert lib.cape_gconv_dw_batch_plan(C.addressof(a64), 1, None, 0, info) == -1


@pytest.mark.parametrize("seed", range(6))
def test_random_item_lists(seed):
    """Up to 12 items of 1-4 sources: lists that need several launches (the argument table holds 6 items / 12 sources), odd batch
    sizes, vertex counts that are no multiple of the 32-row chunk, partial 128-tiles, split counts that are no multiple of 8."""
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
    rows, info = check_plan(shapes, N)
    nsrc_total = sum(len(s[0]) for s in shapes)
    assert info[0] >= max(-(-len(shapes) // 6), -(-nsrc_total // 12))
