"""Lane-level numpy emulation of knn_kernel's list logic (csrc/knn.hip: one wave, one centre): the
bitonic sort and merges, the pending buffer and the stale k-th key, checked against the referee
tests/_knn_ref.py, and the counts DESIGN.md section 7c quotes (steps, admitted keys, sort + merge
passes per centre).  No GPU:  python tools/knn_emulate.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _knn_ref, _np_ref  # noqa: E402

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
lane = np.arange(64)


def shfl_xor(v, j):
    return v[lane ^ j]


def sort64(v):
    k = 2
    while k <= 64:
        j = k >> 1
        while j >= 1:
            o = shfl_xor(v, j)
            up = (lane & k) == 0
            lower = (lane & j) == 0
            v = np.where(up == lower, np.minimum(v, o), np.maximum(v, o))
            j >>= 1
        k <<= 1
    return v


def finish(v):
    j = 32
    while j >= 1:
        o = shfl_xor(v, j)
        v = np.where((lane & j) == 0, np.minimum(v, o), np.maximum(v, o))
        j >>= 1
    return v


def merge64(best, add, high):
    rev = add[63 - lane]
    low = np.minimum(best, rev)
    if high:
        add = finish(np.maximum(best, rev))
    best = finish(low)
    return best, add


def wave(centre, xyz, nsample, TILE=1024):
    wide = nsample > 64
    n = xyz.shape[0]
    lo = np.full(64, EMPTY); hi = np.full(64, EMPTY); kth = EMPTY
    pend = np.zeros(128, np.uint64); npend = 0
    d_all = _np_ref.sqdist(centre[None, :], xyz) if n else np.zeros(0, np.float32)
    stats = dict(steps=0, merges=0, cands=0)

    def merge(v):
        nonlocal lo, hi, kth
        stats['merges'] += 1
        v = sort64(v)
        if wide:
            lo, v = merge64(lo, v, True)
            hi, _ = merge64(hi, v, False)
            kth = hi[nsample - 65]
        else:
            lo, _ = merge64(lo, v, False)
            kth = lo[nsample - 1]

    for base in range(0, n, TILE):
        cnt = min(TILE, n - base)
        for s in range(0, cnt, 64):
            stats['steps'] += 1
            p = s + lane
            valid = p < cnt
            gi = np.where(valid, base + p, 0)
            key = np.where(valid, (d_all[gi].view(np.uint32).astype(np.uint64) << np.uint64(32)) | gi.astype(np.uint64), EMPTY)
            cand = key < kth
            if cand.any():
                rank = np.cumsum(cand) - cand
                pend[npend + rank[cand]] = key[cand]
                npend += int(cand.sum()); stats['cands'] += int(cand.sum())
                assert npend < 128
                if npend >= 64:
                    merge(pend[:64].copy())
                    carry = pend[64:128].copy()
                    npend -= 64
                    pend[:npend] = carry[:npend]
    if npend > 0:
        merge(np.where(lane < npend, pend[:64], EMPTY))
    keys = np.concatenate([lo, hi])[:nsample] if wide else lo[:nsample]
    idx = np.where(keys == EMPTY, 0, keys & np.uint64(0xFFFFFFFF)).astype(np.int32)
    d = np.where(keys == EMPTY, np.float32(1e10), (keys >> np.uint64(32)).astype(np.uint32).view(np.float32))
    return idx, d.astype(np.float32), stats


rng = np.random.default_rng(0)
for (n, m, k, lattice) in [(64, 4, 1, 0), (100, 4, 16, 0), (257, 4, 64, 0), (300, 4, 65, 0), (1000, 3, 100, 0),
                           (500, 3, 128, 0), (10, 3, 16, 0), (512, 8, 32, 1), (70, 2, 128, 0), (2500, 3, 64, 0),
                           (2500, 2, 128, 1), (40000, 1, 64, 0)]:
    if lattice:
        xyz = rng.integers(0, 4, (n, 3)).astype(np.float32); cen = rng.integers(0, 4, (m, 3)).astype(np.float32)
    else:
        xyz = rng.random((n, 3)).astype(np.float32); cen = rng.random((m, 3)).astype(np.float32)
    wi, wd = _knn_ref.knn(cen, xyz, k)
    for c in range(m):
        gi, gd, st = wave(cen[c], xyz, k)
        assert np.array_equal(gi, wi[c]) and np.array_equal(gd.view(np.uint32), wd[c].view(np.uint32)), (n, m, k, c)
    per_step = sum(1 - np.exp(-k / j) for j in range(1, st['steps'] + 1))
    print(f'ok n={n} m={m} k={k} lattice={lattice} last centre: {st}; '
          f'steps a sort-per-step design would sort on (expected, uniform cloud): {per_step:.0f}')
