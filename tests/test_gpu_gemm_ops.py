"""The dense mat-mat layer on the device, kernel by kernel, through the test entry eps_test_gemm_op
(epsilon_amd._solve.gemm_op): Gemm and GemmBatched of csrc/kernels_gemm.hip, kernels_gemm_f64.hip and
kernels_gemv_multi.hip, and MatCopy, AddDiag, SymmetrizeFromLower, ColAbsSums and KronDense of
csrc/kernels_vec.hip.

Kernels and routes (the name is what k::GemmLastRoute reports; every case asserts the one its row
names, so a moved threshold shows as a failure and not as a row that quietly tests something else):

  small          GemmSmallKernel<T>: Gemm, gemm=auto, no lower_only, 1 <= M, N <= 256, K <= 4096 (K = 0
                 included); 32 x 32 blocks, k in chunks of 32.  Rows: SMALL_SHAPES.
  generic        GemmGenericKernel<T>: gemm=generic; gemm=auto when M < 64, N < 64 or K < 32 and the
                 product is not small; f64 under gemm=auto with an odd ld or operand offset; f32 only
                 under gemm=generic or below 64/64/32.  64 x 64 tiles, k slabs of 16.  Rows: GENERIC_*.
  mfma_f32       GemmMfmaF32Kernel (f32): gemm=mfma_simple; gemm=mfma, or gemm=auto from 64/64/32, when
                 lda, ldb or a batch stride of A or B is no multiple of 4 or A or B is not 16-byte
                 aligned.  128 x 128 tiles, k slabs of 32.  Rows: MFMA_F32_*.
  mfma_f32_pipe  GemmMfmaF32PipeKernel<CA, CB> (f32, aligned): gemm=mfma at any size, gemm=auto from
                 64/64/32 when not small.  Slabs of 32 (K = 0, 31, 32, 64, 96, 97); a slab's loads are unchecked (`FAST`) when slab
                 kt + 2 is a whole one of a tile whose window lies inside the operands; an edge tile of
                 an operand with at least 128 rows shifts its window back to end at the edge unless the
                 operand is contiguous along that index and the size is no multiple of 4.
                 Rows: pipe_rows(4, ...).
  mfma_f64       GemmMfmaF64Kernel (f64): gemm=mfma_simple; gemm=mfma with an odd lda, ldb or A / B
                 stride, or A or B not 16-byte aligned.  Rows: MFMA_F64_*.
  mfma_f64_pipe  GemmMfmaF64PipeKernel<CA, CB> (f64, even lds and strides, aligned): gemm=mfma at any
                 size, gemm=auto from 64/64/32 when not small.  Slabs of 8 (K = 0, 7, 8, 16, 24, 25); the window
                 rule with 2 for 4.
                 Rows: pipe_rows(2, ...).
  split_k        the split over K in Gemm(): no lower_only, at most 64 tiles of 128 x 128, K >= 8192
                 (so min(K / 2048, 512 / tiles) >= 2 parts), not taken by an earlier route: batched
                 products into partial results, ReducePartials, and for ldc != M a column-by-column
                 Axpby.  Rows: SPLIT_K_*.
  multi_gemv_n / multi_gemv_t   MultiGemvNKernel / MultiGemvTKernel<4 | 8 | 12 | 16> (f32): B not
                 transposed, no lower_only, N <= 16, M K >= 2^18, ldc == M, A 16-byte aligned with
                 lda % 4 == 0, and for a transposed A the same of B.  Tried BEFORE the gemm option is
                 looked at, so gemm=generic does not keep a product away from it.  Rows: MULTI_*.
  f16split       kernels_gemm_f16split.hip (f32, gemm=auto, M, N >= 1024, K >= 256, M N K >= 8e9): left
                 to tests/test_gpu_parity.py, which holds it to its own accuracy model.  Here only
                 F16_EDGE: a product at the M, N edge with K one short must not report it (its
                 multiply-add count is what keeps it out: a product that one condition alone excludes is
                 far past the sizes of this file).

Left where they are: the split-f16 kernels (above), and the SYRK tail split (SyrkTailFixupKernel and
the kchunk form of the f32 pipe kernel), which needs more than 512 lower tiles and K >= 8192 - a
4160 x 8200 operand - and stays with test_gemm_mfma_vs_oracle of tests/test_gpu_parity.py.  The
syrk_2d and gemm_small options are read once per process, so the 2-D lower_only grid of the f32 pipe
kernel is entered through batch == 2, which takes it whatever the option says.

Every case is the smallest shape that enters one branch.  A test is one row of a table - a kernel, a
gemm option and a shape - in one dtype; the row's transposes, (alpha, beta) pairs, leading dimensions,
offsets and strides run inside it and every one that fails is reported.  Every case asserts:

  * the result is inside the forward error bound (below) of the fp64 reference,
  * both guards, the padding rows M..ldc-1 of every column of C and the gaps between batch members are
    bit-identical to what was placed there,
  * with beta == 0 the result, pre-filled with NaN, comes back finite (C is never read),
  * NaN in the padding rows of every column of A and B and in the gaps between their batch members
    leaves the result finite (they are never read),
  * lower_only: the entries with i >= j are inside the bound, and every tile strictly above the block
    diagonal of the kernel's tile size, pre-filled with NaN, is bit-identical to what was placed - also
    with beta == 1, so it is not read either,
  * a second identical call returns identical bits (no kernel here uses atomics),
  * the route is the one the row names.

Reference and bound.  The inputs are rounded to the tested dtype first; the reference is the fp64
numpy product of the rounded inputs.  alpha and beta are exact in f32.  Per entry

    tol_ij = gamma(K + 8) (|alpha| (|op A| |op B|)_ij + |beta| |C_ij|),  gamma(q) = q u / (1 - q u),

u = 2^-24 (f32) / 2^-53 (f64): the standard forward bound of a sum of K products in any order, fused
or not - the split over K, MultiGemv's partials and the SYRK orders included, since any summation
tree over K leaves is at most K - 1 deep.  ColAbsSums accumulates in fp64: gamma(rows + 8) with
u = 2^-53 over sum |a|.  MatCopy and KronDense are one rounding, u |alpha a| and u |a b|.  AddDiag is
one rounding of the sum, u |w + alpha d|: with a vector d the cases use alpha = -0.5, a power of two,
so that alpha d_i is exact whether or not the compiler fuses it.  SymmetrizeFromLower is exact.  No
tolerance here is measured, none is widened by a factor; tests/test_gemm_op_bound.py checks on the CPU
that evaluations of every case in the tested precision, in three orders, stay inside these bounds.

The largest input is the 70 x 8200 matrix of the split over K; the largest result the 1026 x 1026 one
of the lower_only cases with T = 9 tile rows (45 tiles: the triangular decode past small indices).
"""

import collections
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = 8               # _solve.DENSE_OP_GUARD
SENTINEL = -777.25  # _solve.DENSE_OP_SENTINEL
CPAD = -555.5       # what the padding rows of C and the gaps between its batch members hold
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NP_DT = {"f32": np.float32, "f64": np.float64}

# op, the gemm option, transposes, sizes, alpha, beta, ld - rows of (A, B, C), element offsets of
# (A, B, C), batch, outer, which stride is zero, lower_only, {dtype: route}, the branch the row enters
Case = collections.namedtuple("Case", "op mode ta tb M N K alpha beta pad off batch outer shared lower routes note")

TT = [(0, 0), (0, 1), (1, 0), (1, 1)]
AB4 = [(1.0, 0.0), (-0.75, 0.0), (1.25, 0.5), (-1.0, 1.0)]
BOTH = ("f32", "f64")


def routes(name, dtypes=BOTH):
    return {dt: name for dt in dtypes} if isinstance(name, str) else dict(name)


def case(op, mode, M, N, K, tt=(0, 0), ab=AB4[2], pad=(0, 0, 0), off=(0, 0, 0), batch=1, outer=1, shared="",
         lower=False, route=None, note=""):
    return Case(op, mode, int(tt[0]), int(tt[1]), M, N, K, float(ab[0]), float(ab[1]), tuple(pad), tuple(off),
                batch, outer, shared, lower, routes(route) if route is not None else {dt: "" for dt in BOTH}, note)


def case_id(c):
    s = "%s-%s-%s%s-%dx%dx%d" % (c.op, c.mode, "nt"[c.ta], "nt"[c.tb], c.M, c.N, c.K)
    if any(c.pad):
        s += "-ld+%d%d%d" % c.pad
    if any(c.off):
        s += "-off%d%d%d" % c.off
    if c.batch * c.outer > 1:
        s += "-b%dx%d" % (c.batch, c.outer)
    if c.shared:
        s += "-" + c.shared
    if c.lower:
        s += "-lower"
    return s + "-a%g-b%g" % (c.alpha, c.beta)


def stored(c):
    """(rows, cols) of A and of B as they are stored."""
    return ((c.K, c.M) if c.ta else (c.M, c.K)) + ((c.N, c.K) if c.tb else (c.K, c.N))


def align_pad(dims, V):
    """The padding of (A, B) that makes lda and ldb multiples of V (what the pipe kernels need)."""
    ar, _, br, _ = dims
    return ((-ar) % V, (-br) % V)


def dims_of(M, N, K, tt):
    return ((K, M) if tt[0] else (M, K)) + ((N, K) if tt[1] else (K, N))


def over_tt(op, mode, shapes, route, abs_=(AB4[2], AB4[1]), tts=TT, V=1, **kw):
    """Every shape under every transpose combination and both epilogues (beta != 0, beta == 0), lda
    and ldb padded up to multiples of V."""
    out = []
    for M, N, K, note in shapes:
        for tt in tts:
            pa, pb = align_pad(dims_of(M, N, K, tt), V)
            for ab in abs_:
                out.append(case(op, mode, M, N, K, tt=tt, ab=ab, pad=(pa, pb, 0), route=route, note=note, **kw))
    return out


# ---- GemmSmallKernel -------------------------------------------------------------------------------
SMALL_SHAPES = [
    (1, 1, 1, "one workgroup, one entry, one product"),
    (1, 1, 0, "K == 0: the k loop is not entered, C = beta C"),
    (32, 32, 32, "one whole 32 x 32 block, one whole k chunk"),
    (33, 31, 33, "ragged 32-blocks (2 x 1, the second with one row) and a k-chunk tail of one"),
    (256, 256, 40, "the upper edge of SmallGemmWanted: 8 x 8 blocks"),
]
SMALL_CASES = over_tt("gemm", "auto", SMALL_SHAPES, "small")
SMALL_CASES += [case("gemm", "auto", 257, 8, 8, tt=tt, ab=ab, route="generic",
                     note="M = 257 is past SmallGemmWanted and N < 64: the generic kernel, not `small`")
                for tt in ((0, 0), (1, 1)) for ab in (AB4[2], AB4[1])]

# ---- GemmGenericKernel -----------------------------------------------------------------------------
GENERIC_SHAPES = [
    (1, 1, 1, "one 64 x 64 tile with one entry, one k slab with one row"),
    (64, 64, 16, "one whole tile, one whole k slab of 16"),
    (65, 63, 17, "ragged tiles (2 x 1) and a k slab tail of one"),
    (65, 63, 0, "K == 0: no slab, C = beta C"),
]
GENERIC_CASES = over_tt("gemm", "generic", GENERIC_SHAPES, "generic")
GENERIC_CASES += over_tt("gemm", "auto", [(257, 63, 32, "gemm=auto, not small (M > 256), N < 64: generic"),
                                          (257, 257, 31, "gemm=auto, not small, K < 32: generic")], "generic",
                         tts=((0, 0), (1, 1)))

# ---- GemmMfmaF32Kernel (unpipelined) ---------------------------------------------------------------
MFMA_F32_SHAPES = [
    (1, 1, 1, "one 128 x 128 tile with one entry, one k slab with one row"),
    (128, 128, 32, "one whole tile, one whole k slab of 32"),
    (129, 127, 33, "ragged tiles (2 x 1) and a k slab tail of one"),
    (129, 127, 0, "K == 0: no slab, C = beta C"),
]
MFMA_F32_CASES = over_tt("gemm", "mfma_simple", MFMA_F32_SHAPES, routes("mfma_f32", ("f32",)))
# gemm=auto at 64/64/32 and past `small`, with an lda that is no multiple of 4: A stored 257 x 32
# (lda 257) or, transposed, 32 x 257 with lda 33
MFMA_F32_CASES += [case("gemm", "auto", 257, 64, 32, tt=tt, ab=ab, pad=(1 if tt[0] else 0, 0, 0),
                        route=routes("mfma_f32", ("f32",)),
                        note="gemm=auto from 64/64/32, lda = %d: the unpipelined kernel" % (33 if tt[0] else 257))
                   for tt in TT for ab in (AB4[2], AB4[1])]
MFMA_F32_CASES += [case("gemm", "mfma", 129, 127, 33, tt=tt, ab=AB4[2], pad=align_pad(dims_of(129, 127, 33, tt), 4) + (0,),
                        off=off, route=routes("mfma_f32", ("f32",)),
                        note="gemm=mfma, lda and ldb multiples of 4 but %s one element off alignment" % name)
                   for tt in TT for off, name in (((1, 0, 0), "A"), ((0, 1, 0), "B"))]

# ---- GemmMfmaF64Kernel (unpipelined) ---------------------------------------------------------------
MFMA_F64_SHAPES = [
    (1, 1, 1, "one 128 x 128 tile with one entry, one k slab (16) with one row"),
    (129, 127, 17, "ragged tiles (2 x 1) and a k slab tail of one"),
    (129, 127, 0, "K == 0: no slab, C = beta C"),
]
MFMA_F64_CASES = over_tt("gemm", "mfma_simple", MFMA_F64_SHAPES, routes("mfma_f64", ("f64",)))
MFMA_F64_CASES += over_tt("gemm", "mfma", [(129, 127, 17, "gemm=mfma with an odd lda (129, or 17 transposed): "
                                            "GemmF64Pipe declines")], routes("mfma_f64", ("f64",)))
MFMA_F64_CASES += [case("gemm", "auto", 257, 127, 33, tt=tt, ab=AB4[2], route=routes("generic", ("f64",)),
                        note="f64 gemm=auto with an odd ld: GemmF64Pipe declines and the generic kernel runs")
                   for tt in TT]


# ---- the pipelined kernels -------------------------------------------------------------------------
def pipe_rows(V, SK, dtype, route):
    """The rows of GemmMfma{F32,F64}PipeKernel: V values per 16-byte load, k slabs of SK (the kernel's
    MK: 32 in kernels_gemm.hip, 8 in kernels_gemm_f64.hip); nfull = K / SK, nk = ceil(K / SK)."""
    r = routes(route, (dtype,))
    EVEN, ODD = 128 + V, 130 if V == 4 else 129  # past one tile: a multiple of V, and not one
    shapes = [
        (128, 128, 0, "K == 0: no slab, C = beta C"),
        (128, 128, SK - 1, "nfull = 0, nk = 1: only a checked tail of SK - 1, load(1) loads nothing"),
        (128, 128, SK, "one whole slab: nfull = 1, no FAST slab"),
        (128, 128, 2 * SK, "two whole slabs: nfull = 2, kt + 2 < nfull never holds"),
        (128, 128, 3 * SK, "three whole slabs: slab 0 is the first FAST one (kt + 2 < nfull)"),
        (128, 128, 3 * SK + 1, "three whole slabs and a tail of one: FAST, then checked loads of the tail"),
        (8, 128, 2 * SK + 6, "M = 8, below a tile: no shifted window (M < 128), checked loads of A throughout"),
        (128, 8, 2 * SK + 6, "N = 8, below a tile: checked loads of B throughout"),
        (EVEN, 128, 2 * SK + 6, "M a multiple of V past a tile: the edge tile shifts its window back by 128 - V "
                                   "rows under every transpose and stores only its own V rows"),
        (128, EVEN, 2 * SK + 6, "the same on N"),
        (ODD, 128, 2 * SK + 6,
         "M no multiple of V, lda padded to one: CA (A not transposed) takes checked loads in the edge tile, "
         "!CA the shifted window"),
        (128, ODD, 2 * SK + 6, "the same on N: CB (B transposed) checked, !CB shifted"),
        (164, 128, 2 * SK + 6, "a window shifted back by 92 rows: the rows 36..127 that both tiles load sit in different "
                               "32-row blocks of the two, so an edge tile that stored outside its own rows would meet "
                               "the neighbour's beta epilogue at another time"),
        (128, 164, 2 * SK + 6, "the same on N"),
        (EVEN, ODD, 2 * SK + 6, "both edges at once: a corner tile with a shifted window in i "
                                                     "and a checked or shifted one in j"),
    ]
    out = over_tt("gemm", "mfma", shapes, r, V=V)
    out += over_tt("gemm", "auto", [(257, 64, max(SK, 32), "gemm=auto from 64/64/32 and past `small`, aligned: the "
                                     "pipelined kernel; three row tiles, the last a one-row edge (checked when CA)")],
                   r, V=V)
    return out


PIPE_F32_CASES = pipe_rows(4, 32, "f32", "mfma_f32_pipe")  # K = 0, 31, 32, 64, 96, 97; edges at K = 70
PIPE_F64_CASES = pipe_rows(2, 8, "f64", "mfma_f64_pipe")   # K = 0, 7, 8, 16, 24, 25; edges at K = 22

# ---- the split over K in Gemm() --------------------------------------------------------------------
SPLIT_K_SHAPES = [
    (70, 33, 8192, "one tile, 4 parts of 2048, no remainder: one batched launch, ReducePartials"),
    (70, 33, 8200, "kc = 2112: 3 whole parts and a remainder part of 1864 from a second launch"),
]
SPLIT_K_CASES = over_tt("gemm", "auto", SPLIT_K_SHAPES, "split_k")
SPLIT_K_CASES += [case("gemm", "auto", M, N, K, tt=tt, ab=ab, pad=(0, 0, 3), route="split_k",
                       note="ldc = M + 3: the partials are added into a contiguous S, then C column by column "
                            "through Axpby (beta applied there)")
                  for M, N, K, _ in SPLIT_K_SHAPES for tt in TT for ab in (AB4[2], AB4[3], AB4[1])]

# ---- MultiGemv -------------------------------------------------------------------------------------
MULTI_N = [1, 4, 5, 8, 9, 12, 13, 16]  # both edges of each width class <4>, <8>, <12>, <16>
MULTI_CASES = []
for _n in MULTI_N:
    for _ab in (AB4[2], AB4[1]):
        MULTI_CASES.append(case("gemm", "auto", 1028, _n, 256, tt=(0, 0), ab=_ab,
                                route={"f32": "multi_gemv_n", "f64": "generic"},
                                note="f32: MultiGemvN, two row blocks (the second with one active thread) and 4 K "
                                     "slices of 64; f64: not small (M > 256), N < 64: generic"))
        MULTI_CASES.append(case("gemm", "auto", 33, _n, 8192, tt=(1, 0), ab=_ab,
                                route={"f32": "multi_gemv_t", "f64": "split_k"},
                                note="f32: MultiGemvT, 9 groups of 4 columns of A (the last with one) and two K "
                                     "slices of 4096; f64: the split over K"))
MULTI_CASES += [
    case("gemm", "auto", 1028, 17, 256, route="generic", note="N = 17 is past MultiGemv: generic (N < 64)"),
    case("gemm", "auto", 33, 17, 8192, tt=(1, 0), route="split_k", note="N = 17 is past MultiGemv: the split over K"),
    case("gemm", "generic", 1028, 8, 256, route={"f32": "multi_gemv_n", "f64": "generic"},
         note="gemm=generic does not keep an f32 product from MultiGemv: it is tried before the option is read"),
    case("gemm", "auto", 1028, 8, 256, tt=(0, 1), route="generic",
         note="a transposed B is not MultiGemv's: generic (N < 64)"),
]
for _ab in (AB4[2], AB4[3], AB4[1]):
    MULTI_CASES += [
        case("gemm", "auto", 1028, 8, 256, ab=_ab, pad=(0, 0, 1), route="generic",
             note="ldc = M + 1: MultiGemv declines, generic"),
        case("gemm", "auto", 33, 8, 8192, tt=(1, 0), ab=_ab, pad=(0, 0, 1), route="split_k",
             note="ldc = M + 1: MultiGemv declines, the split over K with its column-by-column Axpby"),
        case("gemm", "auto", 1028, 8, 256, ab=_ab, off=(1, 0, 0), route="generic",
             note="A one element off alignment: MultiGemv declines, generic"),
        case("gemm", "auto", 33, 8, 8192, tt=(1, 0), ab=_ab, off=(1, 0, 0), route="split_k",
             note="A one element off alignment: MultiGemv declines, the split over K"),
        case("gemm", "auto", 33, 8, 8192, tt=(1, 0), ab=_ab, off=(0, 1, 0),
             route="split_k", note="transposed A with B one element off alignment: MultiGemv declines"),
        case("gemm", "auto", 1028, 8, 256, ab=_ab, off=(0, 1, 0), route={"f32": "multi_gemv_n", "f64": "generic"},
             note="A not transposed: MultiGemvN reads B entry by entry, its alignment does not matter"),
    ]

# ---- one product just outside the split-f16 route --------------------------------------------------
F16_EDGE_CASES = [case("gemm", "auto", 1024, 1024, 255, tt=(0, 1), ab=AB4[1], route=routes("mfma_f32_pipe", ("f32",)),
                       note="M, N at GemmSplitF16's 1024 and K one short of its 256, but it is the multiply-add count "
                            "(2.7e8 against 8e9) that alone keeps this product out: a product that only one of the "
                            "three conditions excludes has operands of millions of entries.  Not f16split")]

# ---- variants: (alpha, beta), leading dimensions, element offsets ----------------------------------
# per kernel: the gemm option, the values per 16-byte load its alignment rule counts in (1: none), one
# interior and one ragged shape, the route, and the route an operand that breaks the rule falls to
VARIANT_SHAPES = [
    ("auto", 1, BOTH, [(32, 32, 32), (33, 31, 33)], "small", "small"),
    ("generic", 1, BOTH, [(64, 64, 16), (65, 63, 17)], "generic", "generic"),
    ("mfma_simple", 1, ("f32",), [(128, 128, 32), (129, 127, 33)], "mfma_f32", "mfma_f32"),
    ("mfma", 4, ("f32",), [(128, 128, 64), (132, 130, 70)], "mfma_f32_pipe", "mfma_f32"),
    ("mfma_simple", 1, ("f64",), [(128, 128, 16), (129, 127, 17)], "mfma_f64", "mfma_f64"),
    ("mfma", 2, ("f64",), [(128, 128, 16), (130, 129, 22)], "mfma_f64_pipe", "mfma_f64"),
    ("auto", 1, BOTH, [(70, 33, 8200)], "split_k", "split_k"),
]


def variant_cases():
    out = []
    for mode, V, dtypes, shapes, route, fallback in VARIANT_SHAPES:
        # the padding of a 16-byte load: 4 values in f32, 2 in f64; a kernel that runs in both gets both
        W = 2 if dtypes == ("f64",) else 4
        placements = [((0, 0, 0), (0, 0, 0), "ld == rows"), ((W, W, W), (0, 0, 0), "every ld padded by %d" % W)]
        if dtypes == BOTH:
            placements.append(((2, 2, 2), (0, 0, 0), "every ld padded by 2"))
        placements += [((1, 0, 0), (0, 0, 0), "lda padded by 1"), ((0, 1, 0), (0, 0, 0), "ldb padded by 1"),
                      ((0, 0, 1), (0, 0, 0), "ldc padded by 1"),
                      ((0, 0, 0), (1, 0, 0), "A at an odd element offset"), ((0, 0, 0), (0, 1, 0), "B at an odd offset"),
                      ((0, 0, 0), (0, 0, 1), "C at an odd offset"), ((W, W, W), (1, 1, 1), "all padded, all offset")]
        for M, N, K in shapes:
            for p, (extra, off, pnote) in enumerate(placements):
                for j, ab in enumerate(AB4):
                    # two transpose combinations per (placement, (alpha, beta)): AB4 holds two pairs with
                    # beta == 0 and two with beta != 0, so every placement meets each of the two epilogues
                    # under all four combinations
                    for tt in (TT[(p + j) % 4], TT[(p + j + 2) % 4]):
                        pa, pb = align_pad(dims_of(M, N, K, tt), V)
                        breaks = V > 1 and (extra[0] % V or extra[1] % V or off[0] or off[1])
                        out.append(case("gemm", mode, M, N, K, tt=tt, ab=ab,
                                        pad=(pa + extra[0], pb + extra[1], extra[2]), off=off,
                                        route=routes(fallback if breaks else route, dtypes),
                                        note="%s: %s%s" % (route, pnote, ", which the 16-byte loads cannot take: " +
                                                           fallback if breaks else "")))
    return out


VARIANT_CASES = variant_cases()

# ---- lower_only ------------------------------------------------------------------------------------
# the kernels that take it: the gemm option, the tile, values per 16-byte load, the k slab, dtypes, route.
# K = 2 slabs + 1: two whole slabs and a tail of one (the unpipelined f64 kernel has slabs of 16, so the
# 65 it shares with the f32 one is four slabs and a tail of one there)
LOWER_KERNELS = [
    ("generic", 64, 1, 16, BOTH, "generic", "2-D grid with the early return in both forms"),
    ("mfma_simple", 128, 1, 32, BOTH, {"f32": "mfma_f32", "f64": "mfma_f64"},
     "2-D grid with the early return in both forms"),
    ("mfma", 128, 4, 32, ("f32",), "mfma_f32_pipe",
     "batch == 1: the compact 1-D grid and its sqrt decode; batch == 2: 2-D"),
    ("mfma", 128, 2, 8, ("f64",), "mfma_f64_pipe",
     "batch == 1: the compact 1-D grid and its sqrt decode; batch == 2: 2-D"),
]


def lower_tile(c):
    return 64 if c.mode == "generic" else 128


def lower_cases():
    out = []
    for mode, tile, V, slab, dtypes, route, form in LOWER_KERNELS:
        # T = 1, 2, 3 tile rows (1, 3, 6 lower tiles), ragged, and T = 9 (45 tiles)
        sizes = [(tile - 3, "T = 1: one tile"), (tile + 2, "T = 2: 3 lower tiles, a two-row edge"),
                 (2 * tile + 1, "T = 3: 6 lower tiles, a one-row edge"), (8 * tile + 2, "T = 9: 45 lower tiles")]
        for n, snote in sizes:
            for (op, batch) in (("gemm", 1), ("gemm_batched", 2)):
                if batch == 2 and n > 2 * tile + 1:
                    continue  # the 2-D form has no decode to exercise; T = 9 stays with batch == 1
                for tt, ab in (((0, 1), AB4[3]), ((1, 0), AB4[1])):
                    K = 2 * slab + 1
                    pa, pb = align_pad(dims_of(n, n, K, tt), V)
                    out.append(case(op, mode, n, n, K, tt=tt, ab=ab, pad=(pa, pb, 3), batch=batch, lower=True,
                                    route=routes(route, dtypes), note="lower_only, %s; %s" % (snote, form)))
    return out


LOWER_CASES = lower_cases()

# ---- GemmBatched: batch = 3, outer = 2 -------------------------------------------------------------
BATCH_KERNELS = [
    ("generic", 1, BOTH, (65, 63, 17), "generic"),
    ("mfma_simple", 1, ("f32",), (129, 127, 33), "mfma_f32"),
    ("mfma", 4, ("f32",), (132, 130, 70), "mfma_f32_pipe"),
    ("mfma_simple", 1, ("f64",), (129, 127, 17), "mfma_f64"),
    ("mfma", 2, ("f64",), (130, 129, 22), "mfma_f64_pipe"),
]
BATCH_SHARED = [("", "all five strides past their contiguous values"), ("sA0", "sA == 0: one A per outer index"),
                ("sB20", "sB2 == 0: the B of an inner index is shared by both outer ones")]


def batched_cases():
    out = []
    for mode, V, dtypes, (M, N, K), route in BATCH_KERNELS:
        for shared, snote in BATCH_SHARED:
            for ab in (AB4[2], AB4[1]):
                for tt in TT:
                    pa, pb = align_pad(dims_of(M, N, K, tt), V)
                    out.append(case("gemm_batched", mode, M, N, K, tt=tt, ab=ab, pad=(pa, pb, 1), batch=3, outer=2,
                                    shared=shared, route=routes(route, dtypes),
                                    note="%s, batch 3 x outer 2 (z1 = z %% 3, z2 = z / 3), %s; sC leaves a gap" % (
                                        route, snote)))
        # a batch of 3 alone: outer == 1, the strides of the second level unused
        out.append(case("gemm_batched", mode, M, N, K, ab=AB4[2], pad=align_pad(dims_of(M, N, K, (0, 0)), V) + (0,),
                        batch=3, route=routes(route, dtypes), note="%s, a batch of 3, outer == 1" % route))
    return out


BATCHED_CASES = batched_cases()

GEMM_CASES = (SMALL_CASES + GENERIC_CASES + MFMA_F32_CASES + MFMA_F64_CASES + PIPE_F32_CASES + PIPE_F64_CASES +
              SPLIT_K_CASES + MULTI_CASES + F16_EDGE_CASES + VARIANT_CASES + LOWER_CASES + BATCHED_CASES)

# ---- the helpers of kernels_vec.hip ----------------------------------------------------------------
HELPER_SIZES = [1, 31, 32, 33, 65]
MAT_COPY_CASES = [case("mat_copy", "auto", r, c_, 0, tt=(t, 0), ab=(a, 0.0), pad=(3, 0, 0),
                       note="32 x 32 blocks, %s; a padded source" % ("through the LDS transpose" if t else "straight"))
                  for r in HELPER_SIZES for c_ in HELPER_SIZES for t in (0, 1) for a in (1.0, 0.5, -1.0)]
ADD_DIAG_CASES = [case("add_diag", "auto", n, n, 0, ab=(-0.5 if withd else 1.25, 0.0), pad=(0, 0, 3), batch=withd,
                       note="%d workgroup(s) of 256, ld = n + 3, %s" % ((n + 255) // 256, "alpha d_i" if withd else "alpha"))
                  for n in (1, 256, 257) for withd in (1, 0)]
SYMMETRIZE_CASES = [case("symmetrize", "auto", n, n, 0, pad=(0, 0, p),
                         note="%s, ldc = n + %d" % ("n == 1: no launch" if n == 1 else
                                                    "%d x %d blocks of 32" % ((n + 31) // 32, (n + 31) // 32), p))
                    for n in (1, 2, 32, 33, 65) for p in (0, 3)]
COL_ABS_SUMS_CASES = [case("col_abs_sums", "auto", r, c_, 0, pad=(3, 0, 0),
                           note="one workgroup per column; " + rnote)
                      for r, rnote in ((1, "one lane, the tail branch"), (255, "the tail branch, one idle lane"),
                                       (256, "the tail branch, every lane"), (257, "one two-way round in lane 0 only"),
                                       (1000, "two-way rounds, then a tail in the lanes below 232"))
                      for c_ in (1, 3)]
# kron(a, b): a is M x N, b is K x batch
KRON_CASES = [case("kron", "auto", 1, 1, 3, batch=2, note="a scalar times 3 x 2: one workgroup"),
              case("kron", "auto", 3, 2, 5, batch=7, note="15 x 14 outputs, every index split non-trivial"),
              case("kron", "auto", 33, 9, 17, batch=15, note="561 x 135 outputs: more than 256 x 256, 296 workgroups")]
HELPER_CASES = MAT_COPY_CASES + ADD_DIAG_CASES + SYMMETRIZE_CASES + COL_ABS_SUMS_CASES + KRON_CASES

ALL_CASES = GEMM_CASES + HELPER_CASES


# ---- layout, data, reference and bound -------------------------------------------------------------

def gamma(q, u):
    return q * u / (1.0 - q * u)


def span(rows, cols, ld):
    return 0 if rows == 0 or cols == 0 else (cols - 1) * ld + rows


def cells(off, rows, cols, ld):
    """The flat indices of a rows x cols matrix with leading dimension ld that starts at off."""
    return off + np.arange(rows)[:, None] + ld * np.arange(cols)[None, :]


def up4(x):
    return (x + 3) // 4 * 4


def layout(c):
    """Leading dimensions and, for a batch, strides: every one past its contiguous value, those of A
    and B multiples of 4 (the pipelined kernels' rule), sC with an odd gap after each result."""
    ar, ac, br, bc = stored(c)
    L = dict(lda=ar + c.pad[0], ldb=br + c.pad[1], ldc=c.M + c.pad[2], sA=0, sB=0, sC=0, sA2=0, sB2=0)
    if c.op == "gemm_batched":
        one_a, one_b = up4(L["lda"] * ac) + 4, up4(L["ldb"] * bc) + 4
        L["sA"], L["sA2"] = (0, one_a) if c.shared == "sA0" else (one_a, c.batch * one_a + 8)
        L["sB"], L["sB2"] = (one_b, 0) if c.shared == "sB20" else (one_b, c.batch * one_b + 12)
        L["sC"] = L["ldc"] * c.N + 5
    return L


def make_data(c, dtype):
    """The operands of a gemm case, seeded by its id and rounded to the tested dtype (held as
    float64): per batch member z the matrices A[z], B[z] (as stored) and C[z]; the flat buffers as
    the device gets them - NaN in everything that must not be read - and, per member, the flat
    indices of its result."""
    rng = np.random.RandomState(zlib.crc32(case_id(c).encode()) & 0x7FFFFFFF)

    def randn(*shape):
        return rng.randn(*shape).astype(NP_DT[dtype]).astype(np.float64)

    ar, ac, br, bc = stored(c)
    L = layout(c)
    nz = c.batch * c.outer
    offs_a = [(z % c.batch) * L["sA"] + (z // c.batch) * L["sA2"] for z in range(nz)]
    offs_b = [(z % c.batch) * L["sB"] + (z // c.batch) * L["sB2"] for z in range(nz)]
    d = dict(L=L, A=[], B=[], C=[], idx=[])
    for name, offs, rows, cols, ld in (("A", offs_a, ar, ac, L["lda"]), ("B", offs_b, br, bc, L["ldb"])):
        one = span(rows, cols, ld)
        buf = np.full(max(offs) + one if one else 0, np.nan)
        at = {}
        for o in offs:
            if o not in at:
                at[o] = randn(rows, cols)
                if one:
                    buf[cells(o, rows, cols, ld)] = at[o]
            d[name].append(at[o])
        d[name.lower()] = buf
    one_c = span(c.M, c.N, L["ldc"])
    cbuf = np.full((nz - 1) * L["sC"] + one_c if one_c else 0, CPAD)
    blk = np.arange(c.M) // lower_tile(c)
    above = blk[:, None] < blk[None, :] if c.lower else np.zeros((c.M, c.N), dtype=bool)
    for z in range(nz):
        C0 = randn(c.M, c.N)
        idx = cells(z * L["sC"], c.M, c.N, L["ldc"])
        placed = C0 if c.beta != 0 else np.full((c.M, c.N), np.nan)
        cbuf[idx] = np.where(above, np.nan, placed)
        d["C"].append(C0)
        d["idx"].append(idx)
    d["c"], d["above"] = cbuf, above
    return d


def op_of(X, t):
    return X.T if t else X


def reference(c, d, z):
    """(reference, |alpha| |op A| |op B| + |beta| |C|) of batch member z, in fp64."""
    A, B, C0 = op_of(d["A"][z], c.ta), op_of(d["B"][z], c.tb), d["C"][z]
    ref = c.alpha * A.dot(B)
    mag = abs(c.alpha) * np.abs(A).dot(np.abs(B))
    if c.beta != 0:
        ref = ref + c.beta * C0
        mag = mag + abs(c.beta) * np.abs(C0)
    return ref, mag


def tolerance(c, mag, dtype):
    return gamma(c.K + 8, U[dtype]) * mag


def gemm_kwargs(c, d):
    L = d["L"]
    kw = dict(M=c.M, N=c.N, K=c.K, trans_a=c.ta, trans_b=c.tb, alpha=c.alpha, beta=c.beta, lda=L["lda"], ldb=L["ldb"],
              ldc=L["ldc"], a=d["a"], b=d["b"], c=d["c"], a_off=c.off[0], b_off=c.off[1], c_off=c.off[2],
              lower_only=c.lower)
    if c.op == "gemm_batched":
        kw.update(batch=c.batch, outer=c.outer, sA=L["sA"], sB=L["sB"], sC=L["sC"], sA2=L["sA2"], sB2=L["sB2"])
    return kw


# ---- the checks -------------------------------------------------------------------------------------

def same_bits(x, y):
    """Elementwise: equal, NaN counting as equal to NaN (the dtype round trip keeps no payload)."""
    return (x == y) | (np.isnan(x) & np.isnan(y))


class Configured(object):
    """The dtype and gemm options for one case, restored on the way out."""

    def __init__(self, solve_mod, dtype, mode):
        self.s, self.dtype, self.mode = solve_mod, dtype, mode

    def __enter__(self):
        self.s.set_option("dtype", self.dtype)
        self.s.set_option("gemm", self.mode)

    def __exit__(self, *exc):
        self.s.set_option("gemm", "auto")
        self.s.set_option("dtype", "f32")


def split_guards(c, out, n):
    assert out.shape == (n + 2 * G,), "%s: %d values returned, %d expected" % (case_id(c), out.size, n + 2 * G)
    lo, body, hi = out[:G], out[G:G + n], out[G + n:]
    assert np.array_equal(lo, np.full(G, SENTINEL)), "%s: store below the result: %r" % (case_id(c), lo)
    assert np.array_equal(hi, np.full(G, SENTINEL)), "%s: store past the result: %r" % (case_id(c), hi)
    return body


def check_entries(c, what, got, ref, tol, where=None):
    where = np.ones(got.shape, dtype=bool) if where is None else where
    fin = np.isfinite(got) | ~where
    assert np.all(fin), "%s (%s) %s: %d entries not finite (something that must not be read was)" % (
        case_id(c), c.note, what, np.count_nonzero(~fin))
    with np.errstate(invalid="ignore"):
        bad = np.argwhere(where & ~(np.abs(got - ref) <= tol))
    assert bad.size == 0, "%s (%s) %s: %d entries outside the bound, first at %r: got %r, reference %r, bound %r" % (
        case_id(c), c.note, what, len(bad), tuple(bad[0]), got[tuple(bad[0])],
        np.broadcast_to(ref, got.shape)[tuple(bad[0])], np.broadcast_to(tol, got.shape)[tuple(bad[0])])


def run_gemm_case(solve_mod, c, dtype):
    d = make_data(c, dtype)
    kw = gemm_kwargs(c, d)
    with Configured(solve_mod, dtype, c.mode):
        first, route = solve_mod.gemm_op(c.op, **kw)
        again, route2 = solve_mod.gemm_op(c.op, **kw)
    assert route == c.routes[dtype] and route2 == route, "%s (%s): route %r, the row names %r" % (
        case_id(c), c.note, route, c.routes[dtype])
    body = split_guards(c, first, d["c"].size)
    untouched = np.ones(body.size, dtype=bool)
    low = np.arange(c.M)[:, None] >= np.arange(c.N)[None, :] if c.lower else None
    for z, idx in enumerate(d["idx"]):
        untouched[idx[~d["above"]]] = False
        ref, mag = reference(c, d, z)
        check_entries(c, "member %d" % z, body[idx], ref, tolerance(c, mag, dtype), low)
    keep = same_bits(body[untouched], d["c"][untouched])
    assert np.all(keep), "%s (%s): %d elements of the padding rows, the gaps or the tiles above the block diagonal " \
                         "changed, first at flat index %d" % (case_id(c), c.note, np.count_nonzero(~keep),
                                                              np.nonzero(untouched)[0][np.argmin(keep)])
    assert np.all(same_bits(first, again)), "%s (%s): two runs differ in %d entries" % (
        case_id(c), c.note, np.count_nonzero(~same_bits(first, again)))
    return body


def row_key(c):
    return (c.op, c.mode, c.M, c.N, c.K, c.lower, c.batch, c.outer)


def gemm_params(cases):
    """One test per row of the table and dtype - a kernel, a gemm option and a shape; its transposes,
    (alpha, beta), leading dimensions, offsets and strides run inside it, every failure reported."""
    rows = collections.OrderedDict()
    for c in cases:
        for dt in BOTH:
            if dt in c.routes:
                rows.setdefault(row_key(c) + (dt,), []).append(c)
    ids = ["%s-%s-%dx%dx%d%s%s-%s" % (k[0], k[1], k[2], k[3], k[4], "-lower" if k[5] else "",
                                      "-b%dx%d" % (k[6], k[7]) if k[6] * k[7] > 1 else "", k[8]) for k in rows]
    return pytest.mark.parametrize("row,dtype", [(r, k[8]) for k, r in rows.items()], ids=ids)


def run_gemm_row(solve_mod, row, dtype):
    failures = []
    for c in row:
        try:
            run_gemm_case(solve_mod, c, dtype)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), len(row), "\n".join(failures))


@gemm_params(SMALL_CASES)
def test_gemm_small(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


@gemm_params(GENERIC_CASES)
def test_gemm_generic(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


@gemm_params(MFMA_F32_CASES)
def test_gemm_mfma_f32(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


@gemm_params(MFMA_F64_CASES)
def test_gemm_mfma_f64(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


@gemm_params(PIPE_F32_CASES)
def test_gemm_mfma_f32_pipe(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


@gemm_params(PIPE_F64_CASES)
def test_gemm_mfma_f64_pipe(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


@gemm_params(SPLIT_K_CASES)
def test_gemm_split_k(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


@gemm_params(MULTI_CASES)
def test_gemm_multi_gemv(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


@gemm_params(F16_EDGE_CASES)
def test_gemm_below_the_f16split_threshold(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


@gemm_params(VARIANT_CASES)
def test_gemm_variants(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


@gemm_params(LOWER_CASES)
def test_gemm_lower_only(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


@gemm_params(BATCHED_CASES)
def test_gemm_batched(solve_mod, row, dtype):
    run_gemm_row(solve_mod, row, dtype)


def test_k_zero_is_exact(solve_mod):
    """K == 0: exactly beta C (0.5 scales without rounding), exactly 0 under beta == 0."""
    for c in [c for c in GEMM_CASES if c.K == 0]:
        for dtype in c.routes:
            d = make_data(c, dtype)
            body = run_gemm_case(solve_mod, c, dtype)
            assert np.array_equal(body[d["idx"][0]], c.beta * d["C"][0] if c.beta != 0 else np.zeros((c.M, c.N)))


# ---- the helpers ------------------------------------------------------------------------------------

def helper_data(c, dtype):
    """The operands of a helper case rounded to the tested dtype, the keyword arguments of gemm_op
    (NaN in the padding rows of a source, CPAD in those of a result), and reference, tolerance and the
    flat indices of the result."""
    rng = np.random.RandomState(zlib.crc32(case_id(c).encode()) & 0x7FFFFFFF)
    u = U[dtype]

    def randn(*shape):
        return rng.randn(*shape).astype(NP_DT[dtype]).astype(np.float64)

    def padded(mat, ld, fill):
        rows, cols = mat.shape
        buf = np.full(span(rows, cols, ld), fill)
        buf[cells(0, rows, cols, ld)] = mat
        return buf

    M, N = c.M, c.N
    if c.op == "mat_copy":
        src = randn(N, M) if c.ta else randn(M, N)
        lda = src.shape[0] + c.pad[0]
        ref = c.alpha * op_of(src, c.ta)
        kw = dict(M=M, N=N, trans_a=c.ta, alpha=c.alpha, lda=lda, a=padded(src, lda, np.nan), c=np.full(M * N, np.nan))
        return dict(kw=kw, ref=ref, tol=u * np.abs(ref), idx=cells(0, M, N, M), placed=kw["c"])
    if c.op == "add_diag":
        W, dv = randn(M, M), randn(M)
        ldc = M + c.pad[2]
        inc = c.alpha * dv if c.batch else np.full(M, c.alpha)
        ref = W + np.diag(inc)
        kw = dict(M=M, N=M, alpha=c.alpha, ldc=ldc, c=padded(W, ldc, CPAD), d=dv if c.batch else None)
        return dict(kw=kw, ref=ref, tol=u * np.abs(ref) * np.eye(M), idx=cells(0, M, M, ldc), placed=kw["c"], W=W)
    if c.op == "symmetrize":
        W = randn(M, M)
        ldc = M + c.pad[2]
        start = np.where(np.triu(np.ones((M, M), dtype=bool), 1), np.nan, W)
        ref = np.tril(W) + np.tril(W, -1).T
        kw = dict(M=M, N=M, ldc=ldc, c=padded(start, ldc, CPAD))
        return dict(kw=kw, ref=ref, tol=np.zeros((M, M)), idx=cells(0, M, M, ldc), placed=kw["c"], W=W)
    if c.op == "col_abs_sums":
        A = randn(M, N)
        lda = M + c.pad[0]
        mag = np.abs(A).sum(axis=0)
        kw = dict(M=M, N=N, lda=lda, a=padded(A, lda, np.nan))
        return dict(kw=kw, ref=mag, tol=gamma(M + 8, U["f64"]) * mag, idx=np.arange(N), placed=None)
    if c.op == "kron":
        A, B = randn(M, N), randn(c.K, c.batch)
        ref = np.kron(A, B)
        rows, cols = ref.shape
        kw = dict(M=M, N=N, K=c.K, batch=c.batch, a=A.flatten(order="F"), b=B.flatten(order="F"),
                  c=np.full(rows * cols, np.nan))
        return dict(kw=kw, ref=ref, tol=u * np.abs(ref), idx=cells(0, rows, cols, rows), placed=kw["c"])
    raise ValueError(c.op)


def run_helper_case(solve_mod, c, dtype):
    h = helper_data(c, dtype)
    with Configured(solve_mod, dtype, "auto"):
        first, route = solve_mod.gemm_op(c.op, **h["kw"])
        again, _ = solve_mod.gemm_op(c.op, **h["kw"])
    assert route == ""
    n = c.N if c.op == "col_abs_sums" else h["placed"].size
    body = split_guards(c, first, n)
    got = body[h["idx"]]
    check_entries(c, c.op, got, h["ref"], h["tol"])
    if h["placed"] is not None:
        untouched = np.ones(n, dtype=bool)
        untouched[h["idx"]] = False
        assert np.all(same_bits(body[untouched], h["placed"][untouched])), "%s: the padding rows changed" % case_id(c)
    assert np.all(same_bits(first, again)), "%s: two runs differ" % case_id(c)
    return h, got


def helper_params(cases):
    return pytest.mark.parametrize("c", cases, ids=[case_id(c) for c in cases])


@pytest.fixture(params=["f64", "f32"])
def dtype_both(request):
    return request.param


@pytest.mark.parametrize("rows", HELPER_SIZES)
def test_mat_copy(solve_mod, dtype_both, rows):
    for c in MAT_COPY_CASES:
        if c.M == rows:
            h, got = run_helper_case(solve_mod, c, dtype_both)
            # scaling by 1, 0.5 or -1 does not round
            assert np.array_equal(got, h["ref"]), "%s: the copy is not exact" % case_id(c)


@helper_params(ADD_DIAG_CASES)
def test_add_diag(solve_mod, dtype_both, c):
    h, got = run_helper_case(solve_mod, c, dtype_both)
    off_diag = ~np.eye(c.M, dtype=bool)
    assert np.array_equal(got[off_diag], h["W"][off_diag]), "%s: an off-diagonal entry changed" % case_id(c)


@helper_params(SYMMETRIZE_CASES)
def test_symmetrize_from_lower(solve_mod, dtype_both, c):
    h, got = run_helper_case(solve_mod, c, dtype_both)
    assert np.array_equal(got, got.T), "%s: the result is not bitwise symmetric" % case_id(c)
    assert np.array_equal(np.tril(got), np.tril(h["W"])), "%s: the lower triangle changed" % case_id(c)


@helper_params(COL_ABS_SUMS_CASES)
def test_col_abs_sums(solve_mod, dtype_both, c):
    run_helper_case(solve_mod, c, dtype_both)


@helper_params(KRON_CASES)
def test_kron_dense(solve_mod, dtype_both, c):
    run_helper_case(solve_mod, c, dtype_both)
