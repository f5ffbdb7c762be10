"""NumPy model of the edge stream of `load_synthetic`, written from the
documented behaviour of GpuContext::gen_synthetic and gen_edges_kernel
(KERNELS.md "The synthetic generator's contract"). It does not call into the
engine.

Edge i in [0, ne), all integer arithmetic mod 2^64:

    scale  = smallest k with 2^k >= nv
    t_a, t_ab, t_abc = trunc(a * 65536), trunc((a + b) * 65536),
                       trunc((a + b + c) * 65536)          (fp64 products)
    h = mix64(seed ^ (i * 0x9E3779B97F4A7C15))
    for each of the `scale` levels, most significant bit first:
        every fourth level, starting with the first:
            bits = h;  h = mix64(h + 0x632BE59BD9B4E019)
        r = bits & 0xFFFF;  bits >>= 16
        quad = 0 if r < t_a else 1 if r < t_ab else 2 if r < t_abc else 3
        s = 2 s + (quad >> 1);  d = 2 d + (quad & 1)
    fold:      if s >= nv: s -= nv          (same for d; 2^scale < 2 nv)
    scramble:  x -> (scr_a * x + scr_b) % nv, then swap the images 0 and
               scr_b, so that raw vertex 0 keeps id 0
        scr_a = trunc(nv * 0.6180339887498949), at least 2, bumped until
                coprime with nv
        scr_b = (seed * 0x9E3779B97F4A7C15 mod 2^64) % nv
        no scramble for nv <= 2 or GRAPEHIP_SCRAMBLE=0
    weight:    x = (h >> 16) & 0xFFFFFF, from the h left by the last refill
               (the first h when scale is 0): w = x * (99 / 2^24) + 1 in fp32

mix64 is the splitmix64 step: z += 0x9E3779B97F4A7C15, then the finalizer
(xor-shift 30, * 0xBF58476D1CE4E5B9, xor-shift 27, * 0x94D049BB133111EB,
xor-shift 31).

The weight's rounding. The source expression is an fp32 multiply followed by
an fp32 add, which a compiler may contract to one fused multiply-add. The two
differ on about 1 % of edges (1,633 of 160,000 at nv 20000, ne 160000,
seed 7). The kernel as built for gfx950 uses the FUSED form: one rounding of
the exact x * 99 * 2^-24 + 1. tests/test_gpu_synthetic_oracle.py holds every
stored weight of every shape to that form (a mix of the two would fail), and
the model takes it as its default. 99 * 2^-24 is exact in fp32 and the exact
sum needs at most 31 significant bits, so fp64 computes it without error and
one conversion to fp32 is the fused result.

An undirected graph stores both orientations of every edge with the same
weight, a self-loop twice; a directed graph stores (s, d) in the out-CSR and
(d, s) in the in-CSR."""
from math import gcd

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
REFILL = 0x632BE59BD9B4E019
PHI = 0.6180339887498949
_U = np.uint64


def mix64(z):
    """splitmix64 step on a uint64 array (wraps mod 2^64)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _U(GOLDEN)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def mix64_int(z):
    """mix64 on one Python int."""
    z = (z + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def scale_of(nv):
    scale = 0
    while (1 << scale) < nv:
        scale += 1
    return scale


def thresholds(a=0.57, b=0.19, c=0.19):
    return (int(a * 65536.0), int((a + b) * 65536.0),
            int((a + b + c) * 65536.0))


def scramble_params(nv, seed, scramble=True):
    """(scr_a, scr_b); scr_a == 0 means no scramble."""
    if not scramble or nv <= 2:
        return 0, 0
    scr_a = max(int(nv * PHI), 2)
    while gcd(scr_a, nv) != 1:
        scr_a += 1
    return scr_a, ((seed * GOLDEN) & M64) % nv


def scramble_ids(x, nv, seed, scramble=True):
    """The scramble of folded ids x (any integer array), as int64."""
    x = np.asarray(x, dtype=np.uint64)
    scr_a, scr_b = scramble_params(nv, seed, scramble)
    if scr_a == 0:
        return x.astype(np.int64)
    # scr_a, x < nv < 2^32: the product fits 64 bits
    y = (_U(scr_a) * x + _U(scr_b)) % _U(nv)
    out = np.where(y == _U(scr_b), _U(0), np.where(y == _U(0), _U(scr_b), y))
    return out.astype(np.int64)


def weight_of_bits(x, fused=True):
    """fp32 weight of the 24-bit draw x. fused: one rounding of the exact
    x * 99 * 2^-24 + 1; otherwise the product is rounded to fp32 first."""
    x = np.asarray(x)
    c32 = np.float32(99.0) / np.float32(16777216.0)  # exact: 99 * 2^-24
    if fused:
        return (x.astype(np.float64) * np.float64(c32) + 1.0).astype(
            np.float32)
    return x.astype(np.float32) * c32 + np.float32(1.0)


def raw_stream(nv, ne, seed, a=0.57, b=0.19, c=0.19):
    """(s, d, h) before the fold: ids in [0, 2^scale) as int64 and the final
    hash state as uint64."""
    t_a, t_ab, t_abc = thresholds(a, b, c)
    i = np.arange(ne, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = mix64(_U(seed & M64) ^ (i * _U(GOLDEN)))
    s = np.zeros(ne, dtype=np.int64)
    d = np.zeros(ne, dtype=np.int64)
    bits = np.zeros(ne, dtype=np.uint64)
    for level in range(scale_of(nv)):
        if level % 4 == 0:
            bits = h
            with np.errstate(over="ignore"):
                h = mix64(h + _U(REFILL))
        r = (bits & _U(0xFFFF)).astype(np.int64)
        bits = bits >> _U(16)
        quad = (r >= t_a).astype(np.int64) + (r >= t_ab) + (r >= t_abc)
        s = (s << 1) | (quad >> 1)
        d = (d << 1) | (quad & 1)
    return s, d, h


def fold_ids(x, nv):
    return np.where(x >= nv, x - nv, x)


def synthetic_edges(nv, ne, seed, weighted, a=0.57, b=0.19, c=0.19,
                    scramble=True, fused=True):
    """(src, dst, w) of the generated edges in original ids, one entry per
    edge i in [0, ne): int64, int64, float32 (w is None when unweighted)."""
    s, d, h = raw_stream(nv, ne, seed, a, b, c)
    src = scramble_ids(fold_ids(s, nv), nv, seed, scramble)
    dst = scramble_ids(fold_ids(d, nv), nv, seed, scramble)
    w = None
    if weighted:
        w = weight_of_bits((h >> _U(16)) & _U(0xFFFFFF), fused)
    return src, dst, w


def edge_int(i, nv, seed, a=0.57, b=0.19, c=0.19, scramble=True):
    """Edge i in plain Python ints, loop for loop as the contract reads:
    (src, dst, 24-bit weight draw). The vectorised model is held to it."""
    t_a, t_ab, t_abc = thresholds(a, b, c)
    h = mix64_int((seed & M64) ^ ((i * GOLDEN) & M64))
    s = d = 0
    avail = bits = 0
    for _ in range(scale_of(nv)):
        if avail == 0:
            bits = h
            h = mix64_int((h + REFILL) & M64)
            avail = 4
        r = bits & 0xFFFF
        bits >>= 16
        avail -= 1
        quad = 0 if r < t_a else 1 if r < t_ab else 2 if r < t_abc else 3
        s = (s << 1) | (quad >> 1)
        d = (d << 1) | (quad & 1)
    if s >= nv:
        s -= nv
    if d >= nv:
        d -= nv
    scr_a, scr_b = scramble_params(nv, seed, scramble)
    if scr_a:
        ss = (scr_a * s + scr_b) % nv
        dd = (scr_a * d + scr_b) % nv
        s = 0 if ss == scr_b else scr_b if ss == 0 else ss
        d = 0 if dd == scr_b else scr_b if dd == 0 else dd
    return s, d, (h >> 16) & 0xFFFFFF
