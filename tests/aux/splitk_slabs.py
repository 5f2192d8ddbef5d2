"""Host copies of the group-major split-K slab layout (GemmP::slab_gm): the addresses the split branch of igemm_epilogue writes and the addresses
k_splitk_reduce_gn_apply reads, in the kernels' own integer arithmetic (csrc/gemm_common.h, csrc/gemm_reduce.hip).  Shared by
tests/test_splitk_slab_map.py (CPU: the map is a bijection, the reducer reads what the epilogue wrote) and tests/test_gpu_splitk_slabs.py."""
import collections

import numpy as np

RGA_MAXR = 8

# the shapes of the slab tests: 3 x 3 convs in front of GroupNorm + SiLU.  split = the split count ASKED for; the dispatcher rounds it to whole
# K tiles (eff_splitk): 4 -> 4, 2 -> 2, 8 -> 5 (9 K tiles), 16 -> 16 (63 K tiles: the reducer's 16-deep batch of loads)
Shape = collections.namedtuple("Shape", "name N H W Cin Cout G bm bn split")
SHAPES = [
    Shape("tile spans both images", 2, 8, 8, 128, 160, 4, 128, 160, 4),
    Shape("4-wide items", 2, 16, 16, 64, 80, 4, 64, 128, 2),
    Shape("ragged last n-tile", 2, 8, 8, 64, 200, 5, 64, 160, 8),
    Shape("16 loads in flight", 1, 16, 16, 448, 160, 4, 64, 160, 16),
]


def eff_splitk(K, split):
    kt = -(-K // 64)
    kps = -(-kt // max(split, 1))
    return -(-kt // kps)


def fast_div_magic(d):
    """(mul, shr) of csrc/gemm_common.h: n / d = (umulhi(mul, n) + n) >> shr."""
    l = 0
    while (1 << l) < d:
        l += 1
    return ((((1 << l) - d) << 32) // d + 1) & 0xFFFFFFFF, l


def fast_div(n, mul, shr):
    n = np.asarray(n, np.uint64)
    return (((np.uint64(mul) * n) >> np.uint64(32)) + n) >> np.uint64(shr)


def formula(m, n, N, HoWo, G):
    """the layout as the documents state it: offset of element (m, n) inside one split's slab."""
    cpg = N // G
    img, g = m // HoWo, n // cpg
    return ((img * G + g) * HoWo + (m - img * HoWo)) * cpg + (n - g * cpg)


def epilogue_offsets(M, N, HoWo, G, bm, bn):
    """[(m, n, offset, width)] of every store the split branch of igemm_epilogue issues into one slab under slab_gm, enumerated the way the kernel
    does -- tiles, the 4 consumer tiles x 2 halves, items of 8 columns -- with its own arithmetic (magic-number divides, the second quad's
    address from the first).  width = elements one store covers (8, or 4 + 4 where cpg % 8 != 0)."""
    cpg = N // G
    hm, hs = fast_div_magic(HoWo)
    cm, cs = fast_div_magic(cpg)
    TM, TN = bm // 2, bn // 2
    ROWS, CPR = TM // 2, TN // 8
    out = []
    for m0 in range(0, M, bm):
        for n0 in range(0, N, bn):
            for w4 in range(4):
                for half in range(2):
                    mb, nb = m0 + (w4 & 1) * TM + half * ROWS, n0 + (w4 >> 1) * TN
                    idx = np.arange(ROWS * CPR)
                    row, c8 = idx // CPR, idx % CPR
                    m, n = mb + row, nb + c8 * 8
                    keep = (m < M) & (n < N)
                    m, n = m[keep].astype(np.int64), n[keep].astype(np.int64)
                    img, g = fast_div(m, hm, hs).astype(np.int64), fast_div(n, cm, cs).astype(np.int64)
                    u = lambda a: np.asarray(a).astype(np.uint32)                        # the kernel forms the offset in 32 bits, unsigned
                    ga, gb = u(HoWo * (N - cpg)), u((HoWo - 1) * cpg)
                    o = u(m) * u(cpg) + u(n) + u(img) * ga + u(g) * gb
                    o1 = np.where(u(n) + u(4) - u(g) * u(cpg) >= u(cpg), o + u(4) + gb, o + u(4))
                    if cpg % 8 == 0:
                        out += [(int(a), int(b), int(d), 8) for a, b, d in zip(m, n, o)]
                    else:
                        out += [(int(a), int(b), int(d), 4) for a, b, d in zip(m, n, o)] + [(int(a), int(b) + 4, int(d), 4) for a, b, d in zip(m, n, o1)]
    return out


def rga_geometry(HoWo, N, G):
    """(CV, RPS) of k_splitk_reduce_gn_apply at gpb == 1 (cpg % 4 == 0), or None."""
    cpg = N // G
    if cpg % 4 or cpg > 256:
        return None
    cv = cpg // 4
    rps = min(1024 // cv, HoWo)
    return (cv, rps) if rps * RGA_MAXR >= HoWo else None


def reducer_reads(nimg, N, HoWo, G, pairs):
    """{(m, n of a quad): (offset the value is LOADED from, thread that ends up holding it)} for every quad the fused reducer consumes: thread
    (rl, v) of block (img, g) holds quad v of rows rl + k RPS.  pairs: the 16-byte form -- the even lane of a lane pair loads both lanes' quads of
    sweep k, the odd lane those of sweep k + 1 (k even), and they swap; also returns the 16-byte load addresses for the alignment check."""
    cpg = N // G
    CV, RPS = rga_geometry(HoWo, N, G)
    S, totq = RPS * CV, HoWo * CV
    got, loads16 = {}, []
    for b in range(nimg * G):
        img, g = divmod(b, G)
        base = b * HoWo * cpg
        for t in range(S):
            rl, v = divmod(t, CV)
            for k in range(RGA_MAXR):
                r = rl + k * RPS
                if r >= HoWo:
                    continue
                if not pairs:
                    off = base + 4 * (t + k * S)
                else:
                    ke, odd_loader = k - (k & 1), k & 1                     # the sweep pair, and which lane of the pair loads sweep k
                    loader = (t & ~1) | odd_loader
                    q = (loader - odd_loader) + (ke + odd_loader) * S       # the kernel's q for the loading lane
                    assert loader < S and q < totq and q % 2 == 0
                    loads16.append(base + 4 * q)
                    off = base + 4 * q + 4 * (t & 1)                        # low half: the even lane's quad, high half: the odd lane's
                got[(img * HoWo + r, g * cpg + 4 * v)] = (off, t)
    return got, loads16


def to_row_major(slab, N, HoWo, G):
    """one group-major slab (M N,) -> row-major (M, N)."""
    M = slab.size // N
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    return slab[formula(m, n, N, HoWo, G)]
