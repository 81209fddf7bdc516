"""The float64 judge of the split-fp16 GEMM family (csrc/batched_nn.hip: gemm_h2, rows_dot, split_planes; no GPU code, no tests;
importable anywhere) and the table of cases test_gemm_split_gpu.py runs, with their seeded operands -- so the CPU file that pins the
judge (test_gemm_split_reference_cpu.py) and the GPU file that uses it see the same numbers.

One call of nnpops_gemm_split is, for every batch entry b,   C_b = epi( pro(A_b) B_b^T ):
    pro 0: A as given                      pro 1: A[m][k] = pv[k] * CELU'(PY[m][k])       (A itself is not read)
    epi 0: none        epi 1: CELU(. + bias)        epi 2: . * CELU'(Y)
with CELU' taken from a saved CELU OUTPUT, y > 0 ? 1 : y / alpha + 1 (continuous at 0: no case sits on a branch), row m of A read
from row a_rows[m] and row m of C written to row c_rows[m] where the maps are given (Y is not mapped), and B the float64 value of the
[N][K] matrix the planes were split from.  `judge` evaluates that in float64.  `witness` repeats the kernels' ALGORITHM on the CPU:
both operands split into hi / lo fp16 planes exactly as BatchedNN._planes does (A after a_scale), hi hi + 2^-11 (hi lo + lo hi) with
float32 accumulation -- what the algorithm itself costs, which the CPU file shows inside half the bar on every row.

The kernel a call runs (nnpops_gemm_split_last) is one of gemm_h2<EPI, PRO, BN, KS, FAST>:
    shape 0  (bn 128, k_split 1)   ceil(N/128) ceil(M/64) batch >= 512
    shape 1  (bn 64,  k_split 1)   otherwise, ceil(N/64) ceil(M/64) batch >= 600     (impossible for N <= 64: the two counts are equal)
    shape 2  (bn 64,  k_split 2)   otherwise: eight waves, the halves of every 64-wide K step added through LDS
    FAST     K % 8 == 0, the leading dimension of A (PY) % 4 == 0, its base 16-byte aligned, with batch > 1 its stride % 4 == 0, under
             the prologue pv 16-byte aligned and its stride % 4 == 0, and NNPOPS_GEMM_FAST not 0
Every row of the table states the kernel it expects; the CPU file checks the statement against its own restatement of the rule, and
that the table holds every reachable (EPI, PRO, shape, FAST) and every edge the issue lists.  The thresholds are reached with `batch`,
not with size: every row is a GEMM of at most a few million multiply-adds.

Buffers: `place` lays a logical operand [nb][rows][width] into a flat buffer, element (b, r, j) at off + b stride + r ld + j, and fills
everything else -- behind every row where ld > width, the rows after the last, the floats in front of a misaligned base -- with NaN
(operands) or SENTINEL (outputs).  By default a row's leading dimensions lie BEYOND its widths (lda = K + 4, ldy = N + 1, ldc = N + 3,
ldb = K rounded up to 32, + 8 with fp16 NaN behind the zero padding); `dense` rows use the widths themselves, as capi.gemm_split does.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

BAR = 4e-6                  # of the judge's largest entry: the bar test_batched_nn_gpu.py holds this kernel to at K up to 2048
ROWS_DOT_BAR = 4e-6         # of the largest sum_k |a_k w_k| over the rows (a float32 sum of <= 2048 terms through a 64-lane tree
                            # stays below about 40 * 2^-24 = 2.4e-6 of it)
E_BAR, G_BAR = 1e-5, 1e-4   # GroupedMLP and the module: the project's end-to-end bars (of max |e| per atom, of max |dE/dx|)
SENTINEL = -7777.25         # (exact in float32; no result of a case comes near it)
TAIL_ROWS = 2               # rows of filler after the last row of every buffer
LO = 2048.0


def up32(v):
    return (v + 31) // 32 * 32


def up4(v):
    return (v + 3) // 4 * 4


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------- arithmetic
def celu(v, alpha):
    return torch.where(v > 0, v, alpha * torch.expm1(v / alpha))


def celu_grad_from_output(y, alpha):
    return torch.where(y > 0, torch.ones_like(y), y / alpha + 1.0)


def split(x):
    """float32 -> (hi, lo) fp16, x = hi + 2^-11 lo: BatchedNN._planes without the padding"""
    hi = x.half()
    lo = ((x - hi.float()) * LO).half()
    return hi, lo


def planes(w, ldb, fill=float("nan")):
    """[nb][N][K] float32 -> hi, lo [nb][N][ldb] fp16: zero padded to K rounded up to 32 (what the kernel reads), `fill` behind"""
    nb, n, k = w.shape
    kpad = up32(k)
    assert ldb >= kpad and ldb % 8 == 0
    out = []
    for part in split(w):
        p = torch.full((nb, n, ldb), fill, dtype=torch.float16)
        p[:, :, :kpad] = 0
        p[:, :, :k] = part
        out.append(p)
    return out


# ---------------------------------------------------------------------------------------------- the table
# expect = (bn, k_split, fast).  Of A: lda / strideA / a_off describe PY under the prologue (A is then not passed).  rows: the rows of
# the A and C buffers where a map picks M of them.  replicas: every operand shared (stride 0), distinct C blocks.  amp: scale of A.
Case = namedtuple("Case", "name section epi pro M N K batch expect lda strideA a_off ldb strideB ldc strideC ldy strideY strideBias "
                          "pv_off stridePv a_scale alpha amp a_rows c_rows rows replicas fast_env seed")

SHAPES = {0: (128, 1), 1: (64, 1), 2: (64, 2)}
VARIANTS = ((0, 0), (1, 0), (2, 0), (0, 1))                 # the plain kernel, each fused epilogue, the prologue
COMBOS = tuple((e, p) for p in (0, 1) for e in (0, 1, 2))
M_EDGES = (1, 63, 64, 65, 129)
N_EDGES = {0: (1, 63, 64, 65, 127, 128, 129),               # 128-wide tile: the second half of the B rows entirely / just out of range
           2: (1, 15, 16, 17, 63, 64, 65),                  # 64-wide tiles: the epilogue skips whole 16-column blocks
           1: (65, 79, 80, 81, 127, 128, 129)}              # shape 1 needs N > 64: its LAST tile is 1, 15, 16, 17, 63, 64, 1 wide
K_FAST = (8, 24, 32, 40, 64, 72, 96, 128)
K_SLOW = (1, 7, 31, 33, 63, 65, 97)
K_SPLIT = (8, 32, 40, 96, 2048)                             # under k_split 2: second half-step never / partly filled, odd steps, many
# (shape, N) cells of the 64-wide edge list no call can reach: with N <= 64 both tile counts are equal, so >= 600 implies >= 512
UNREACHABLE = tuple((1, n) for n in N_EDGES[2] if n <= 64)
# every (epi, pro, shape, fast) is reachable: nothing to list
UNREACHABLE_KERNELS = ()


def _batch(shape, M, N):
    """the batch that puts an (M, N) problem into `shape` (the thresholds are reached with batch, not with size)"""
    tm = cdiv(M, 64)
    if shape == 0:
        return cdiv(512, cdiv(N, 128) * tm)
    if shape == 1:
        assert N > 64
        return cdiv(600, cdiv(N, 64) * tm)
    return 2


_ROWS = []


def _row(name, section, epi, pro, M, N, K, batch, shape, fast, dense=False, lda=None, strideA=None, a_off=0, ldb=None, strideB=None,
         ldc=None, strideC=None, ldy=None, strideY=None, strideBias=None, pv_off=0, stridePv=None, a_scale=1.0, alpha=0.1, amp=1.5,
         a_rows=False, c_rows=False, rows=None, replicas=False, fast_env=None):
    rows = rows if rows is not None else M
    lda = lda if lda is not None else (K if dense else K + 4)
    ldb = ldb if ldb is not None else (up32(K) if dense else up32(K) + 8)
    ldc = ldc if ldc is not None else (N if dense else N + 3)
    ldy = ldy if ldy is not None else (N if dense else N + 1)
    rows_a = rows if a_rows else M
    rows_c = rows if c_rows else M
    if replicas:
        strideA, strideB, strideBias, strideY, stridePv = 0, 0, 0, 0, 0
    strideA = strideA if strideA is not None else up4(rows_a * lda)
    strideB = strideB if strideB is not None else N * ldb
    strideC = strideC if strideC is not None else rows_c * ldc
    strideY = strideY if strideY is not None else M * ldy
    strideBias = strideBias if strideBias is not None else N
    stridePv = stridePv if stridePv is not None else up4(K)
    bn, ks = SHAPES[shape]
    _ROWS.append(Case(name, section, epi, pro, M, N, K, batch, (bn, ks, int(fast)), lda, strideA, a_off, ldb, strideB, ldc, strideC, ldy,
                      strideY, strideBias, pv_off, stridePv, a_scale, alpha, amp, a_rows, c_rows, rows, replicas, fast_env,
                      1000 + len(_ROWS)))


def _tag(epi, pro):
    return f"e{epi}p{pro}"


def _build():
    # ---- a. every kernel once, on dense operands (the layout capi.gemm_split passes): 6 x 3 x 2
    for epi, pro in COMBOS:
        for shape in (0, 1, 2):
            N = 65 if shape == 2 else 129
            for fast, K in ((1, 40), (0, 33)):
                _row(f"a-{_tag(epi, pro)}-s{shape}-f{fast}", "a", epi, pro, 65, N, K, _batch(shape, 65, N), shape, fast, dense=True)
    # ---- b. the tile edges: every value with the plain kernel in every shape; once with each fused epilogue and the prologue, the
    #         shape rotating over the values
    for v, (epi, pro) in enumerate(VARIANTS):
        for i, M in enumerate(M_EDGES):
            for shape in ((0, 1, 2) if v == 0 else ((i + v) % 3,)):
                N = 70 if shape == 1 else 40
                _row(f"b-M{M}-{_tag(epi, pro)}-s{shape}", "bM", epi, pro, M, N, 24, _batch(shape, M, N), shape, 1)
        for i in range(7):                                  # (the others: the 128-wide list in shape 0, the 64-wide one in 2 and 1 in turn)
            for shape in ((0, 1, 2) if v == 0 else (0, 2 - (i + v) % 2)):
                N = N_EDGES[shape][i]
                _row(f"b-N{N}-{_tag(epi, pro)}-s{shape}", "bN", epi, pro, 33, N, 24, _batch(shape, 33, N), shape, 1)
        for i, K in enumerate(K_FAST):
            for shape in ((0, 1, 2) if v == 0 else ((i + v) % 3,)):
                N = 70 if shape == 1 else 40
                _row(f"b-K{K}-{_tag(epi, pro)}-s{shape}", "bK", epi, pro, 33, N, K, _batch(shape, 33, N), shape, 1)
        for i, K in enumerate(K_SLOW):
            for shape in ((0, 1, 2) if v == 0 else ((i + v) % 3,)):
                N = 70 if shape == 1 else 40
                # the plain rows keep lda = K + 4 (odd: scalar loads); the others a multiple of 4, so that the non-FAST branch
                # takes its 16-byte loads for the whole groups of eight and scalar loads for the tail
                _row(f"b-K{K}-{_tag(epi, pro)}-s{shape}", "bK", epi, pro, 33, N, K, _batch(shape, 33, N), shape, 0,
                     lda=None if v == 0 else up4(K) + 4)
    # ---- c. K under the K-splitting kernel, every variant (two tiles in both directions, batch 1)
    for epi, pro in VARIANTS:
        for K in K_SPLIT:
            _row(f"c-K{K}-{_tag(epi, pro)}", "c", epi, pro, 65, 65, K, 1, 2, 1)
    _row("c-K2047-e1p0", "c", 1, 0, 65, 65, 2047, 1, 2, 0)
    # ---- d. every cause of non-FAST on its own, with a fused epilogue or the prologue and batch > 1 (K = 24: FAST but for the cause)
    _row("d-K20", "d", 1, 0, 65, 40, 20, 3, 2, 0)
    _row("d-lda27", "d", 2, 0, 65, 40, 24, 2, 2, 0, lda=27)
    _row("d-base-off1", "d", 1, 0, 65, 40, 24, 2, 2, 0, a_off=1)
    _row("d-base-off1-pro", "d", 0, 1, 65, 40, 24, 2, 2, 0, a_off=1)
    _row("d-strideA", "d", 2, 0, 65, 40, 24, 3, 2, 0, strideA=65 * 28 + 2)
    _row("d-pv-off1", "d", 0, 1, 65, 40, 24, 2, 2, 0, pv_off=1)
    _row("d-stridePv", "d", 2, 1, 65, 40, 24, 2, 2, 0, stridePv=25)
    _row("d-env", "d", 1, 1, 65, 40, 24, 2, 2, 0, fast_env="0")
    _row("d-base-off1-s0", "d", 1, 0, 65, 129, 24, _batch(0, 65, 129), 0, 0, a_off=1)
    _row("d-strideA-s1", "d", 2, 0, 65, 129, 24, _batch(1, 65, 129), 1, 0, strideA=65 * 28 + 1)
    _row("d-batch1-strideA", "d", 1, 0, 65, 40, 24, 1, 2, 1, strideA=65 * 28 + 1)       # (a stride counts only with batch > 1)
    # ---- e. the product's layouts (GroupedMLP): members interleaved in a row; layer 0 through a_rows; the last backward GEMM
    #         through c_rows; a_scale 1/16
    for name, (h1, h2, h3), fast in (("w8", (40, 24, 16), 1), ("odd", (30, 22, 17), 0)):
        mem = 3
        _row(f"e-layer2-{name}", "e", 1, 0, 65, h2, h1, mem, 2, fast, lda=mem * h1, strideA=h1, ldb=up32(h1), strideBias=h2,
             ldc=mem * h2, strideC=h2, a_scale=1.0 / 16)
        _row(f"e-back4-{name}", "e", 2, 1, 65, h2, h3, mem, 2, fast, lda=mem * h3, strideA=h3, stridePv=h3, ldb=up32(h3),
             ldy=mem * h2, strideY=h2, ldc=mem * h2, strideC=h2, a_scale=1.0 / 16)
        _row(f"e-back2-{name}", "e", 2, 0, 65, h1, h2, mem, 2, fast, lda=mem * h2, strideA=h2, ldb=up32(h2),
             ldy=mem * h1, strideY=h1, ldc=mem * h1, strideC=h1, a_scale=1.0 / 16)
        F = 56 if fast else 50
        _row(f"e-layer0-{name}", "e", 1, 0, 65, mem * h1, F, 1, 2, fast, dense=True, a_rows=True, rows=100, a_scale=1.0 / 16)
        _row(f"e-back0-{name}", "e", 0, 0, 65, F, mem * h1, 1, 2, fast, dense=True, c_rows=True, rows=100,
             a_scale=1.0 / 16)
    _row("e-both-maps", "e", 1, 0, 129, 65, 40, 1, 2, 1, a_rows=True, c_rows=True, rows=150)
    # ---- f. a_scale 2^-6 with operands of 3e4 (beyond fp16 without it), in every shape; an alpha besides 0.1
    for shape in (0, 1, 2):
        N = 70 if shape == 1 else 40
        _row(f"f-huge-s{shape}", "f", 0, 0, 65, N, 40, _batch(shape, 65, N), shape, 1, a_scale=2.0 ** -6, amp=3.0e4)
    _row("f-huge-e1", "f", 1, 0, 65, 40, 33, 2, 2, 0, a_scale=2.0 ** -6, amp=3.0e4)
    for epi, pro in ((1, 0), (2, 0), (0, 1), (2, 1)):
        _row(f"f-alpha-{_tag(epi, pro)}", "f", epi, pro, 65, 40, 40, 2, 2, 1, alpha=0.5)
    # ---- g. replicas: one problem as `batch` copies (every operand stride 0, distinct C blocks), at a batch in every shape
    for epi, pro in ((0, 0), (1, 0), (2, 1)):
        _row(f"g-{_tag(epi, pro)}-s0", "g", epi, pro, 65, 129, 40, 128, 0, 1, replicas=True)
        _row(f"g-{_tag(epi, pro)}-s1", "g", epi, pro, 64, 128, 40, 300, 1, 1, replicas=True)
        _row(f"g-{_tag(epi, pro)}-s2", "g", epi, pro, 65, 129, 40, 3, 2, 1, replicas=True)
    # ---- h. the thresholds themselves (K = 8: the work is in the count)
    _row("h-64x64-b511", "h", 0, 0, 64, 64, 8, 511, 2, 1)
    _row("h-64x64-b512", "h", 0, 0, 64, 64, 8, 512, 0, 1)
    _row("h-64x128-b299", "h", 0, 0, 64, 128, 8, 299, 2, 1)
    _row("h-64x128-b300", "h", 0, 0, 64, 128, 8, 300, 1, 1)
    _row("h-64x128-b511", "h", 0, 0, 64, 128, 8, 511, 1, 1)
    _row("h-64x128-b512", "h", 0, 0, 64, 128, 8, 512, 0, 1)


_build()
CASES = {c.name: c for c in _ROWS}
assert len(CASES) == len(_ROWS), "two rows share a name"


def shape_of(case):
    return {v: k for k, v in SHAPES.items()}[case.expect[:2]]


def names(section=None):
    return [c.name for c in _ROWS if section is None or c.section.startswith(section)]


# ---------------------------------------------------------------------------------------------- operands, layout
Operands = namedtuple("Operands", "A PY pv W bias Y a_rows c_rows")     # logical, float32 / int32 CPU tensors (None where unused)


@functools.lru_cache(maxsize=None)
def operands(name):
    """the seeded logical operands of a row: activations O(1) (times amp), weights N(0, 1/sqrt(K)), saved activations CELU outputs;
    computed once, not changed.  A / PY [nb][rows][K], pv [nb][K], W [nb][N][K], bias [nb][N], Y [nb][M][N]; nb = 1 for replicas."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    nb = 1 if c.replicas else c.batch
    rows_a = c.rows if c.a_rows else c.M

    def rnd(*shape):
        return torch.randn(shape, generator=gen)
    A = PY = pv = bias = Y = a_rows = c_rows = None
    if c.pro == 0:
        A = (c.amp * rnd(nb, rows_a, c.K)).float()
    else:
        PY = celu(1.5 * rnd(nb, rows_a, c.K), c.alpha).float()
        pv = (c.amp * rnd(nb, c.K)).float()
    W = (rnd(nb, c.N, c.K) / np.sqrt(c.K)).float()
    if c.epi == 1:
        bias = (0.3 * rnd(nb, c.N)).float()
    if c.epi == 2:
        Y = celu(1.5 * rnd(nb, c.M, c.N), c.alpha).float()
    if c.a_rows:
        a_rows = torch.randperm(c.rows, generator=gen)[:c.M].to(torch.int32)
    if c.c_rows:
        c_rows = torch.randperm(c.rows, generator=gen)[:c.M].to(torch.int32)
    return Operands(A, PY, pv, W, bias, Y, a_rows, c_rows)


def index(nb, rows, width, ld, stride, off, row_map=None):
    """[nb][rows][width] int64: where place() puts element (b, r, j) -- off + b stride + r ld + j, r through row_map where given"""
    r = torch.arange(rows) if row_map is None else row_map.long()
    return off + torch.arange(nb).view(-1, 1, 1) * stride + r.view(1, -1, 1) * ld + torch.arange(width).view(1, 1, -1)


def extent(nb, rows, width, ld, stride, off):
    """the floats of a buffer that holds such an operand and TAIL_ROWS rows of filler after its last element"""
    return off + (nb - 1) * stride + (rows - 1) * ld + width + TAIL_ROWS * ld + 8


def written(idx, size):
    """[size] bool: the places an index names"""
    mask = torch.zeros(size, dtype=torch.bool)
    mask[idx.reshape(-1)] = True
    return mask


def place(x, ld, stride, off, fill, dtype=torch.float32):
    """logical [nb][rows][width] -> flat buffer (see the module docstring); no two elements share a place"""
    nb, rows, width = x.shape
    idx = index(nb, rows, width, ld, stride, off).reshape(-1)
    size = extent(nb, rows, width, ld, stride, off)
    assert int(written(idx, size).sum()) == idx.numel(), "the layout folds two elements onto one place"
    buf = torch.full((size,), fill, dtype=dtype)
    buf[idx] = x.reshape(-1).to(dtype)
    return buf


Buffers = namedtuple("Buffers", "A PY pv Bh Bl bias Y C c_index")       # flat CPU buffers (views from their offsets are the operands)


@functools.lru_cache(maxsize=2)
def buffers(name):
    """a row's operands laid out as the row says, and its output buffer full of SENTINEL; c_index [batch][M][N]: where C lands.
    (Not to be written to: a test copies them to the device.)"""
    c, ops = CASES[name], operands(name)
    nan = float("nan")
    nb = 1 if c.replicas else c.batch
    a_like = ops.A if c.pro == 0 else ops.PY
    a_buf = place(a_like, c.lda, c.strideA, c.a_off, nan)
    pv = place(ops.pv.unsqueeze(1), c.K, c.stridePv, c.pv_off, nan) if c.pro == 1 else None
    hi, lo = planes(ops.W, c.ldb)
    Bh, Bl = (place(p, c.ldb, c.strideB, 0, nan, torch.float16) for p in (hi, lo))
    bias = place(ops.bias.unsqueeze(1), c.N, c.strideBias, 0, nan) if c.epi == 1 else None
    Y = place(ops.Y, c.ldy, c.strideY, 0, nan) if c.epi == 2 else None
    rows_c = c.rows if c.c_rows else c.M
    c_index = index(c.batch, c.M, c.N, c.ldc, c.strideC, 0, ops.c_rows)
    C = torch.full((extent(c.batch, rows_c, c.N, c.ldc, c.strideC, 0),), SENTINEL, dtype=torch.float32)
    assert int(written(c_index, C.numel()).sum()) == c_index.numel(), "two elements of C share a place"
    assert nb in (1, c.batch)
    return Buffers(a_buf if c.pro == 0 else None, a_buf if c.pro == 1 else None, pv, Bh, Bl, bias, Y, C, c_index)


# ---------------------------------------------------------------------------------------------- the judge and the witness
def _rows_of(x, row_map):
    return x if row_map is None else x[:, row_map.long()]


@functools.lru_cache(maxsize=None)
def judge(name):
    """-> C [batch][M][N] float64 numpy, read-only"""
    c, ops = CASES[name], operands(name)
    if c.pro == 0:
        A = _rows_of(ops.A, ops.a_rows).double()
    else:
        A = ops.pv.double().unsqueeze(1) * celu_grad_from_output(_rows_of(ops.PY, ops.a_rows).double(), c.alpha)
    v = torch.matmul(A, ops.W.double().transpose(1, 2))
    if c.epi == 1:
        v = celu(v + ops.bias.double().unsqueeze(1), c.alpha)
    elif c.epi == 2:
        v = v * celu_grad_from_output(ops.Y.double(), c.alpha)
    out = v.expand(c.batch, c.M, c.N).contiguous().numpy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def witness(name):
    """the kernels' algorithm in float32 on the CPU -> C [batch][M][N] float32 numpy, read-only"""
    c, ops = CASES[name], operands(name)
    inv_alpha = np.float32(1.0) / np.float32(c.alpha)
    if c.pro == 0:
        A = _rows_of(ops.A, ops.a_rows)
    else:
        y = _rows_of(ops.PY, ops.a_rows)
        A = ops.pv.unsqueeze(1) * torch.where(y > 0, torch.ones_like(y), y * float(inv_alpha) + 1.0)
    ah, al = (p.float() for p in split(A * np.float32(c.a_scale)))
    wh, wl = (p.float().transpose(1, 2) for p in split(ops.W))
    v = torch.matmul(ah, wh) + np.float32(1.0 / LO) * (torch.matmul(ah, wl) + torch.matmul(al, wh))
    v = v * (np.float32(1.0) / np.float32(c.a_scale))
    if c.epi == 1:
        v = v + ops.bias.unsqueeze(1)
        v = torch.where(v > 0, v, np.float32(c.alpha) * (torch.exp(v * float(inv_alpha)) - 1.0))
    elif c.epi == 2:
        y = ops.Y
        v = v * torch.where(y > 0, torch.ones_like(y), y * float(inv_alpha) + 1.0)
    assert v.dtype == torch.float32
    out = v.expand(c.batch, c.M, c.N).contiguous().numpy()
    out.setflags(write=False)
    return out


def figure(out, ref):
    """(largest error, the judge's largest entry): the row passes when error <= BAR * scale"""
    return float(np.abs(np.asarray(out, dtype=np.float64) - ref).max()), float(np.abs(ref).max())


# ---------------------------------------------------------------------------------------------- rows_dot
ROWS_DOT_M = (1, 3, 4, 5, 9)                                # four rows per workgroup
ROWS_DOT_K_VECTOR = (4, 252, 256, 260, 1280)                # 64 lanes x 4 floats per round
ROWS_DOT_K_SCALAR = (1, 63, 65, 130)
DotCase = namedtuple("DotCase", "name M K lda vector")
DOT_CASES = {}
for _K in ROWS_DOT_K_VECTOR + ROWS_DOT_K_SCALAR:
    for _M in ROWS_DOT_M:
        _vec = _K in ROWS_DOT_K_VECTOR
        DOT_CASES[f"M{_M}-K{_K}"] = DotCase(f"M{_M}-K{_K}", _M, _K, _K + (4 if _vec else 3), _vec)
for _M in ROWS_DOT_M:
    DOT_CASES[f"M{_M}-K256-lda257"] = DotCase(f"M{_M}-K256-lda257", _M, 256, 257, False)     # K % 4 == 0 but lda % 4 != 0: scalar


@functools.lru_cache(maxsize=None)
def dot_operands(name):
    """-> A [M][K], w [K], bias, out_rows (a permutation into 2 M + 3 places); float64 reference, its scale, the float32 witness"""
    c = DOT_CASES[name]
    gen = torch.Generator().manual_seed(5000 + list(DOT_CASES).index(name))
    A = (1.5 * torch.randn((c.M, c.K), generator=gen)).float()
    w = (torch.randn((c.K,), generator=gen) / np.sqrt(c.K)).float()
    bias = 0.375
    out_rows = torch.randperm(2 * c.M + 3, generator=gen)[:c.M].to(torch.int32)
    ref = (A.double() @ w.double() + bias).numpy()
    scale = float((A.double().abs() @ w.double().abs()).max())
    wit = (A @ w + np.float32(bias)).numpy()
    return A, w, bias, out_rows, ref, scale, wit


# ---------------------------------------------------------------------------------------------- split_planes
PlaneCase = namedtuple("PlaneCase", "name rows cols ldw ldp")          # the SOURCE matrix is [rows][cols] in a buffer [rows][ldw]
PLANE_CASES = {c.name: c for c in (
    PlaneCase("5x33", 5, 33, 40, 96),
    PlaneCase("70x50", 70, 50, 53, 64),
    PlaneCase("64x64-dense", 64, 64, 64, 64),
    PlaneCase("1100x1000", 1100, 1000, 1001, 1024),         # > 4096 * 256 plane elements both ways: the grid-stride loop repeats
)}


@functools.lru_cache(maxsize=None)
def plane_source(name):
    """[rows][ldw] float32, NaN behind the columns: magnitudes from below fp16's subnormals (2^-24 = 6e-8) to its largest normals
    (6e4), both signs, some exact zeros"""
    c = PLANE_CASES[name]
    gen = torch.Generator().manual_seed(7000 + list(PLANE_CASES).index(name))
    mag = 10.0 ** (torch.rand((c.rows, c.cols), generator=gen) * 13.5 - 9.0)              # 1e-9 .. 3e4
    w = (mag * torch.randn((c.rows, c.cols), generator=gen).clamp(-2.0, 2.0)).float()
    w[torch.rand((c.rows, c.cols), generator=gen) < 0.02] = 0.0
    buf = torch.full((c.rows, c.ldw), float("nan"))
    buf[:, :c.cols] = w
    return buf


# ---------------------------------------------------------------------------------------------- GroupedMLP and the module
# widths the fused kernels do not take (F % 8 != 0, or a width that is no multiple of 8), three members; a kind without atoms
MlpCase = namedtuple("MlpCase", "name F widths members counts forward_last backward_last")
MLP_CASES = {c.name: c for c in (
    # forward: the last GEMM is layer 4 of the last kind (K = H2, members interleaved); backward: dx = d1 W0 (K = members * H1)
    MlpCase("F50", 50, (30, 22, 18), 3, (1, 64, 0, 65), (64, 2, 0), (64, 2, 0)),
    MlpCase("F1008", 1008, (40, 96, 17), 3, (65, 0, 1, 64), (64, 2, 1), (64, 2, 1)),
)}


def pack_grouped(kinds, split_planes_of):
    """the operands of torch.ops.NNPOpsBatchedNN.GroupedMLP in the layout the op documents, from networks as mlp_float64.networks
    makes them (w0 [M][H1][F] ...); split_planes_of: BatchedNN._planes.  -> fwd_hi, fwd_lo, bwd_hi, bwd_lo, biases, last_w, last_b"""
    fh, fl, bh, bl, biases, last_w, last_b = [], [], [], [], [], [], []
    for kd in kinds:
        M = kd["w0"].shape[0]
        fwd = [kd[w].reshape(-1, kd[w].shape[2]) for w in ("w0", "w2", "w4")]
        bwd = [kd["w0"].reshape(-1, kd["w0"].shape[2]).t().contiguous(),
               torch.cat([kd["w2"][m].t() for m in range(M)], 0).contiguous(),
               torch.cat([kd["w4"][m].t() for m in range(M)], 0).contiguous()]
        for mats, his, los in ((fwd, fh, fl), (bwd, bh, bl)):
            for w in mats:
                hi, lo = split_planes_of(w.float())
                his.append(hi.reshape(-1))
                los.append(lo.reshape(-1))
        biases += [kd[b].reshape(-1) for b in ("b0", "b2", "b4")]
        last_w.append(kd["w6"].reshape(-1))
        last_b.append(float(kd["b6"].double().sum()))
    return torch.cat(fh), torch.cat(fl), torch.cat(bh), torch.cat(bl), torch.cat(biases).float(), torch.cat(last_w).float(), last_b


@functools.lru_cache(maxsize=None)
def mlp_frame(name):
    """-> kinds (with their atoms), x [atoms][F], order (the atoms grouped by kind): seeded, computed once"""
    from mlp_float64 import networks
    c = MLP_CASES[name]
    gen = torch.Generator().manual_seed(9000 + list(MLP_CASES).index(name))
    n = sum(c.counts)
    perm = torch.randperm(n, generator=gen)
    x = torch.randn((n, c.F), generator=gen).abs().float()
    kinds, first = [], 0
    for s, count in enumerate(c.counts):
        kd = networks(c.widths, c.members, c.F, seed=9100 + 10 * list(MLP_CASES).index(name) + s)
        kd["atoms"] = perm[first:first + count].to(torch.int32)
        first += count
        kinds.append(kd)
    return kinds, x, perm.to(torch.int32)
