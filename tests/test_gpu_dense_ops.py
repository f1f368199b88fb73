"""The dense mat-vec layer on the device, launcher by launcher, through the test entry
eps_test_dense_op (epsilon_amd._solve.dense_op): Gemv (N and T), Symv and SymvPacked, ReducePartials,
SumSq / SumSqDiff / Dot, Axpby and DiagMul of csrc/kernels_gemv.hip and csrc/kernels_vec.hip.

Every case is the smallest shape at which one branch of a launcher is entered; the tables below name
the branch per row, read from the launchers' conditions (V = 4 in f32 / 2 in f64 values per 16-byte
load, 256 threads, RC = 12288 / 6144 rows of x in LDS).  Every case asserts:

  * the result is inside the forward error bound (below) of the fp64 reference,
  * the guard elements on both sides of the output are untouched,
  * with beta == 0 the output, pre-filled with NaN, comes back finite (y is never read),
  * NaN in the padding rows rows..lda-1 of every column (and, for Symv, in every 128 x 128 tile
    strictly above the block diagonal) leaves the result finite (they are never read),
  * a second identical call returns identical bits (fixed summation orders).

Reference and bound.  The inputs are rounded to the tested dtype first; the reference is the fp64
numpy result on the rounded inputs.  alpha and beta are exact in f32.  Per entry

    tol_i = gamma(k + 8) * (|alpha| (|A| |x|)_i + |beta| |y_i| + |add_i|),  gamma(q) = q u / (1 - q u),

u = 2^-24 (f32) / 2^-53 (f64), k the contraction length (cols for gemv_n, rows for gemv_t, n for
Symv, nparts for ReducePartials): the standard forward bound, valid for any summation order, with or
without FMA; the + 8 covers the scaling, the beta term and the add term (whose magnitude |add_i| the
last rounding of (alpha sum + beta y) + add scales with).  The reductions accumulate in fp64 whatever
the dtype and products of f32 values are exact in fp64, so their bound is gamma(n + 8) with
u = 2^-53 over sum |terms| (+ |preset| when accumulating).  Axpby and DiagMul are elementwise, three
roundings: 4 u (|a x| + |b y|), against a reference in extended precision (an fp64 one rounds two or
three times itself).  No tolerance here is measured, none is widened by a factor;
tests/test_dense_op_bound.py checks on the CPU that evaluations of every case in the tested precision
stay inside these bounds.

Left to tests/test_gpu_full_size.py: the kNChunk loop of GemvNKernel needs more than 512 columns per
column split, which takes a matrix of about 0.5 GB.
"""

import collections
import math
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = 8               # _solve.DENSE_OP_GUARD
SENTINEL = -777.25  # _solve.DENSE_OP_SENTINEL
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NP_DT = {"f32": np.float32, "f64": np.float64}
SB = 128            # Symv tile

# op, rows (n), cols, lda - rows, offsets of (a, x, y, add), alpha, beta, nparts, with_add, use_work,
# accumulate, alias_xy, the branch the row enters
Case = collections.namedtuple("Case", "op rows cols pad off alpha beta nparts add work acc alias note")


def case(op, rows, cols=0, pad=0, off=(0, 0, 0, 0), ab=(1.0, 0.0), nparts=1, add=False, work=False,
         acc=False, alias=False, note=""):
    return Case(op, rows, cols, pad, tuple(off), float(ab[0]), float(ab[1]), nparts, add, work, acc, alias, note)


def case_id(c):
    s = "%s-%dx%d" % (c.op, c.rows, c.cols) if c.op.startswith("gemv") else "%s-%d" % (c.op, c.rows)
    if c.op == "reduce_partials":
        s += "x%d" % c.nparts
    if c.pad:
        s += "-ld+%d" % c.pad
    if any(c.off):
        s += "-off" + "".join(str(o) for o in c.off)
    s += "-a%g-b%g" % (c.alpha, c.beta)
    for flag, name in ((c.add, "add"), (c.work, "work"), (c.acc, "acc"), (c.alias, "alias")):
        if flag:
            s += "-" + name
    return s


AB4 = [(1.0, 0.0), (-0.75, 0.0), (1.25, 0.5), (-1.0, 1.0)]
AB3 = AB4[:3]
OFF1 = (1, 1, 1, 1)

# ---- GemvN (LaunchGemvN): vector form iff A 16-byte aligned, lda % V == 0 and rows % V == 0; row
# blocks of 256 V rows; column splits = min(ceil(1024 / row_blocks), ceil(cols / 64)), re-derived
# from the columns per split; one split: beta is applied in GemvNKernel, else in GemvNReduceBody
# (splits dealt to 4 waves, per = ceil(splits / 4) each, 8 at a time while 8 are left).
GEMV_N_SHAPES = [
    (1, 1, "scalar form (rows % V != 0), one thread, one column, single launch"),
    (1, 2100, "scalar form, 33 splits of 64 columns: reduce with per = 9, the 8-way loop plus one"),
    (4, 7, "vector form f32 <4> with ONE active thread / f64 <2> with two; tail loop of 7 columns (< 8)"),
    (4, 65, "vector form, two splits of 33 and 32 columns: the unrolled loop then a tail of 1 / none"),
    (257, 7, "scalar form, second row block with one active thread; single launch"),
    (257, 64, "scalar form, 64 columns: a single launch (max_split 1), beta in the matrix kernel, 8 x 8-unrolled"),
    (257, 65, "scalar form, two splits (33, 32), reduce with waves 2 and 3 empty (per = 1)"),
    (1024, 1, "vector form, one full row block in f32 / two in f64; one column"),
    (1024, 64, "vector form, single launch: beta in the vector epilogue"),
    (1024, 65, "vector form, two splits of 33 and 32 columns"),
    (1024, 300, "vector form, 5 splits of 60: the reduce's fourth wave is empty (per = 2: 2, 2, 1, 0)"),
    (1028, 64, "vector form, f32: second row block with a single active thread (rows 1024..1027); f64: 3 blocks"),
    (1028, 2100, "vector form, 33 splits of 64 (the last 52): per = 9 enters the 8-way unrolled reduce loop"),
    (2051, 1, "odd rows: scalar form, 9 row blocks, the last with 3 active threads"),
    (2051, 300, "odd rows: scalar form, 5 splits of 60"),
    (2051, 2100, "odd rows: scalar form, 33 splits"),
]
GEMV_N_VARIANT_SHAPES = [(1024, 300), (1028, 2100)]

# ---- GemvT (LaunchGemvT): vec iff A aligned and lda % V == 0.  GemvT2Kernel<V> (8 columns per pass,
# all rows in LDS) iff vec, rows % V == 0 and 256 V <= rows <= RC; else GemvTKernel<V or 1> (16 columns
# per pass, 4 per wave; x staged in chunks of RC rows when rows > RC).  Grids are capped at 1024 passes.
GEMV_T_SHAPES = [
    (8, 1, "GemvTKernel<V>: rows below 256 V; one column, waves 1..3 idle; nvec = 2 (f32) / 4 (f64)"),
    (8, 7, "GemvTKernel<V>: wave 1 has 3 of its 4 columns, waves 2 and 3 idle"),
    (8, 17, "GemvTKernel<V>: second pass with one column, three idle waves"),
    (8, 33, "GemvTKernel<V>: three passes, the last with one column"),
    (8, 16400, "GemvTKernel<V>: 1025 passes of 16 on a grid of 1024: the grid-stride loop"),
    (1020, 8, "f32: below the T2 edge, GemvTKernel<4> with nvec = 255; f64: GemvT2Kernel<2>, one full pass"),
    (1020, 9, "f32: GemvTKernel<4>; f64: T2 with a tail pass of one column"),
    (1020, 16, "f32: GemvTKernel<4>, one full pass; f64: T2, two full passes"),
    (1024, 1, "lower edge of GemvT2Kernel<4> in f32 (nvec = 256: one load per thread); tail pass only"),
    (1024, 8, "T2: one full pass, no tail"),
    (1024, 9, "T2: the tail pass (one column)"),
    (1024, 17, "T2: two full passes and a tail"),
    (1024, 8200, "T2: 1025 passes of 8 on a grid of 1024: the grid-stride loop"),
    (1027, 3, "odd lda: GemvTKernel<1>, the scalar loop only; one wave with 3 columns"),
    (1027, 16, "odd lda: GemvTKernel<1>, one full pass"),
    (1027, 33, "odd lda: GemvTKernel<1>, three passes"),
    (6144, 8, "f64: the upper edge of T2 (rows == RC); f32: T2"),
    (6144, 9, "f64: the upper edge of T2 with a tail pass"),
    (6146, 3, "f64: GemvTKernel<2>, two chunks (6144 + 2 rows); f32: lda % 4 == 2, GemvTKernel<1>, one chunk"),
    (6146, 17, "f64: two chunks, second pass with three idle waves that still reach the chunk barriers"),
    (12288, 7, "f32: the upper edge of T2 (rows == RC); f64: GemvTKernel<2>, exactly two full chunks"),
    (12288, 9, "f32: the upper edge of T2 with a tail pass; f64: two chunks, three columns idle in wave 2"),
    (12289, 3, "odd: GemvTKernel<1>; f32 two chunks with a one-row second chunk, f64 three chunks"),
    (12289, 16, "odd: GemvTKernel<1>, chunked, one full pass"),
    (12292, 3, "GemvTKernel<V>, chunked, a four-row last chunk; waves past cols still reach the chunk barriers"),
    (12292, 9, "GemvTKernel<V>, chunked; wave 2 has one column, wave 3 none"),
    (12292, 17, "GemvTKernel<V>, chunked, two passes"),
]
GEMV_T_VARIANT_SHAPES = [(1024, 33), (12292, 9)]


def gemv_cases(op, shapes, variant_shapes):
    out = []
    for rows, cols, note in shapes:
        for ab in (AB4[2], AB4[1]):  # beta != 0 and the beta == 0 epilogue
            out.append(case(op, rows, cols, ab=ab, note=note))
    for rows, cols in variant_shapes:
        for pad, pnote in ((0, "lda == rows"), (1, "lda = rows + 1: the scalar form"),
                           (4, "lda = rows + 4: the vector form over padded columns")):
            for off, onote in (((0, 0, 0, 0), "aligned base"), (OFF1, "base offset 1: the scalar form")):
                for ab in AB4:
                    out.append(case(op, rows, cols, pad=pad, off=off, ab=ab, note=pnote + ", " + onote))
    if op == "gemv_t":
        # rows % V != 0 under a vector lda: the 16-byte loop AND the remainder loop of GemvTKernel<V>
        for ab in (AB4[2], AB4[1]):
            out.append(case(op, 1027, 16, pad=1, ab=ab, note="lda = 1028: GemvTKernel<V>, nvec = 256 (f32) / 513 "
                                                              "(f64), then a remainder of 3 / 1 rows"))
            out.append(case(op, 12289, 3, pad=3, ab=ab, note="lda = 12292: GemvTKernel<V>, chunked; the last chunk is "
                                                             "one row, remainder loop only"))
    # an empty matrix: Gemv fills y with 0 (beta == 0) or scales it through Axpby(y, beta, y, 0)
    r0, c0 = (5, 0) if op == "gemv_n" else (0, 5)
    out.append(case(op, r0, c0, ab=(1.0, 0.0), note="empty contraction, beta == 0: zeros"))
    out.append(case(op, r0, c0, ab=(1.0, 0.5), note="empty contraction: 0.5 y by Axpby with x aliasing y"))
    return out


GEMV_N_CASES = gemv_cases("gemv_n", GEMV_N_SHAPES, GEMV_N_VARIANT_SHAPES)
GEMV_T_CASES = gemv_cases("gemv_t", GEMV_T_SHAPES, GEMV_T_VARIANT_SHAPES)

# ---- Symv (LaunchSymv): one workgroup per 128 x 128 tile on or below the diagonal; a tile is loaded
# with 16-byte loads (`full`) iff it lies wholly inside the matrix, lds % 4 == 0 and S is aligned, else
# entry by entry with bounds checks; SymvReduceBody adds the nb partial vectors of a row block in two
# half-workgroups, 8 at a time while 8 are left to a half (both halves from nb = 16).
SYMV_N = [
    (1, "one tile, one entry: the non-full branch, 127 zero rows and columns"),
    (127, "one ragged tile: the non-full branch"),
    (128, "one whole tile: full with lds % 4 == 0 and an aligned base, non-full else"),
    (129, "nb = 2: a whole diagonal tile, an off-diagonal tile of one row (column sums), a 1 x 1 diagonal tile"),
    (257, "nb = 3: whole off-diagonal tiles (non-full: lds is never a multiple of 4 here)"),
]
SYMV_BIG = 1921  # nb = 16: both half-workgroups of SymvReduceBody enter the 8-at-a-time loop
SYMV_EXTRA_LDS = [(257, 3, "lds = 260: whole tiles take the full branch, edge tiles the other"),
                  (SYMV_BIG, 3, "lds = 1924: whole tiles take the full branch, nb = 16")]


def symv_cases():
    out = []
    for n, note in SYMV_N:
        for pad in (0, 1, 4):
            for off in ((0, 0, 0, 0), OFF1):
                for work in (False, True):
                    for ab in AB4:
                        out.append(case("symv", n, n, pad=pad, off=off, ab=ab, work=work, note=note))
    big = "nb = 16: the 8-at-a-time loop of both halves of SymvReduceBody"
    out += [case("symv", SYMV_BIG, SYMV_BIG, pad=0, ab=AB4[2], note=big),
            case("symv", SYMV_BIG, SYMV_BIG, pad=1, ab=AB4[0], work=True, note=big),
            case("symv", SYMV_BIG, SYMV_BIG, pad=4, off=OFF1, ab=AB4[3], note=big),
            case("symv", SYMV_BIG, SYMV_BIG, pad=4, ab=AB4[1], work=True, note=big)]
    for n, pad, note in SYMV_EXTRA_LDS:
        out += [case("symv", n, n, pad=pad, ab=AB4[2], note=note),
                case("symv", n, n, pad=pad, off=OFF1, ab=AB4[1], work=True, note=note + "; base offset 1: non-full")]
    return out


def symv_packed_cases():
    """SymvPack + SymvPacked against Symv on the same operands, every n of the table."""
    out = []
    for n, note in SYMV_N + [(SYMV_BIG, "nb = 16")]:
        i = 0
        for pad in ((0, 1, 4) if n != SYMV_BIG else (0, 4)):
            for off in (((0, 0, 0, 0), OFF1) if n != SYMV_BIG else ((0, 0, 0, 0),)):
                out.append(case("symv_packed", n, n, pad=pad, off=off, ab=AB4[i % 4], work=bool(i % 2),
                                note="packed tiles (always the 16-byte loads) against " + note))
                i += 1
    for n, pad, note in SYMV_EXTRA_LDS:
        out.append(case("symv_packed", n, n, pad=pad, ab=AB4[2], note="packed against the plain full branch, " + note))
    return out


SYMV_CASES = symv_cases()
SYMV_PACKED_CASES = symv_packed_cases()

# ---- ReducePartials: ReducePartials4Kernel (float4; 32 part lanes x 8 row quads, 8 loads in flight
# from 225 partials up) iff f32, rows % 4 == 0, nparts >= 64 and partial, y and add are 16-byte aligned;
# else GemvNReduceKernel (64 rows per workgroup, the partials dealt to 4 waves).
RP_ROWS = [1, 3, 4, 63, 64, 65, 100, 4096]
RP_NPARTS = [
    (1, "generic: per = 1, waves 1..3 empty"),
    (3, "generic: per = 1, wave 3 empty"),
    (4, "generic: one partial per wave"),
    (5, "generic: per = 2, waves hold 2, 2, 1, 0"),
    (29, "generic: per = 8, the 8-way loop in waves 0..2, a tail of 5 in wave 3"),
    (63, "generic: per = 16, two 8-way rounds per wave, one and a tail of 7 in wave 3; the last count below the float4 form"),
    (64, "float4 form in f32 when rows % 4 == 0 (two partials per part lane), generic else"),
    (65, "float4 form: part lane 0 holds three partials; generic: per = 17"),
    (300, "float4 form: the 8-loads-in-flight loop (k + 224 < nparts) then a tail; generic: per = 75"),
]
RP_CASES = [case("reduce_partials", rows, nparts=nparts, add=add, ab=ab, note=note)
            for rows in RP_ROWS for nparts, note in RP_NPARTS for add in (False, True) for ab in AB3]
# the float4 shapes with one operand off by one element: back to the generic form
RP_ALIGN_SHAPES = [(4, 64), (64, 64), (100, 65), (4096, 300)]
RP_ALIGN_OFFS = [((1, 0, 0, 0), "partial"), ((0, 0, 1, 0), "y"), ((0, 0, 0, 1), "add")]
RP_ALIGN_CASES = [case("reduce_partials", rows, nparts=nparts, add=True, ab=AB4[2], off=off,
                       note="float4 shape with %s off by one element: the generic form" % name)
                  for rows, nparts in RP_ALIGN_SHAPES for off, name in [((0, 0, 0, 0), "nothing")] + RP_ALIGN_OFFS]

# ---- SumSq / SumSqDiff / Dot (LaunchRed): one workgroup and one launch up to n = 8192, else a grid of
# min(1024, ceil(n / 8 / 256)) workgroups and a second launch that adds their partials; the slot is
# overwritten or (accumulate) added to.
RED_N = [
    (0, "one launch, nothing read: the slot becomes 0 (or keeps its value)"),
    (1, "one launch, one lane"),
    (255, "one launch, one idle lane"),
    (256, "one launch, every lane one entry"),
    (257, "one launch, lane 0 two entries"),
    (8192, "the last one-launch size: 32 entries per lane, the 4-way loop only"),
    (8193, "the first two-launch size: 4 workgroups, RedFinalKernel"),
    (1000003, "two launches, 489 workgroups, the 4-way grid-stride loop and its tail"),
]
RED_CASES = [case(op, n, acc=acc, note=note) for op in ("sumsq", "sumsq_diff", "dot") for n, note in RED_N
             for acc in (False, True)]
RED_CASES += [case(op, n, acc=True, off=OFF1, note="operands at an odd element offset (no vector loads here)")
              for op in ("sumsq", "sumsq_diff", "dot") for n in (257, 8193)]
PRESET = 3.5

# ---- Axpby / DiagMul (LaunchEw): 16-byte packs iff every operand is aligned and n >= 4 V (16 in f32,
# 8 in f64), then a scalar tail; else entry by entry.  Axpby: b == 0 never reads y (ScaleF),
# b == 1 with a == +-1 is AddF, the rest AxpbyF; DiagMul: b == 0 is DiagMul0F.
EW_N = [
    (0, "no launch"),
    (1, "scalar form"),
    (7, "scalar form (below 4 V in both dtypes)"),
    (8, "f64: the pack form, no tail; f32: scalar"),
    (9, "f64: the pack form with a tail of one; f32: scalar"),
    (16, "f32: the pack form, no tail; f64: 8 packs"),
    (17, "the pack form with a tail of one in both dtypes"),
    (1000003, "pack form: 977 (f32) / 1954 (f64) workgroups and a tail of 3 / 1; entry by entry (odd offset): "
              "the grid capped at 2048 workgroups, the grid-stride loop"),
]
AXPBY_AB = [((-0.75, 0.0), "b == 0: ScaleF, y is NaN"), ((1.0, 1.0), "AddF +"), ((-1.0, 1.0), "AddF -"),
            ((1.25, 0.5), "AxpbyF")]
AXPBY_CASES = [case("axpby", n, ab=ab, off=(0, ox, oy, 0), note=note + "; " + abnote)
               for n, note in EW_N for ox in (0, 1) for oy in (0, 1) for ab, abnote in AXPBY_AB]
AXPBY_CASES += [case("axpby", n, ab=(0.5, 0.0), off=(0, 0, oy, 0), alias=True,
                     note=note + "; x aliases y, b == 0: the call Gemv makes for an empty matrix")
                for n, note in EW_N for oy in (0, 1)]
DIAG_MUL_CASES = [case("diag_mul", n, ab=ab, off=(od, ox, oy, 0), note=note + "; " + abnote)
                  for n, note in EW_N for od in (0, 1) for ox in (0, 1) for oy in (0, 1)
                  for ab, abnote in (((-0.75, 0.0), "b == 0: DiagMul0F, y is NaN"), ((1.25, 0.5), "DiagMulF"))]

ALL_CASES = (GEMV_N_CASES + GEMV_T_CASES + SYMV_CASES + SYMV_PACKED_CASES + RP_CASES + RP_ALIGN_CASES +
             RED_CASES + AXPBY_CASES + DIAG_MUL_CASES)


# ---- data, reference and bound ---------------------------------------------------------------------

def gamma(q, u):
    return q * u / (1.0 - q * u)


def make_data(c, dtype):
    """The operands of case c, seeded by its id, rounded to the tested dtype (held as float64)."""
    rng = np.random.RandomState(zlib.crc32(case_id(c).encode()) & 0x7FFFFFFF)

    def randn(*shape):
        return rng.randn(*shape).astype(NP_DT[dtype]).astype(np.float64)

    d = {}
    n = c.rows
    if c.op in ("gemv_n", "gemv_t"):
        d["A"] = randn(c.rows, c.cols)
        d["x"] = randn(c.cols if c.op == "gemv_n" else c.rows)
        d["y"] = randn(c.rows if c.op == "gemv_n" else c.cols)
    elif c.op in ("symv", "symv_packed"):
        L = np.tril(randn(n, n))
        d["A"] = L + np.tril(L, -1).T
        d["x"], d["y"] = randn(n), randn(n)
    elif c.op == "reduce_partials":
        d["A"] = randn(c.nparts, n)  # partial k is row k
        d["y"] = randn(n)
        if c.add:
            d["add"] = randn(n)
    elif c.op == "sumsq":
        d["x"] = randn(n)
    elif c.op in ("sumsq_diff", "dot"):
        d["x"], d["y"] = randn(n), randn(n)
    elif c.op == "axpby":
        d["y"] = randn(n)
        d["x"] = d["y"] if c.alias else randn(n)
    elif c.op == "diag_mul":
        d["A"], d["x"], d["y"] = randn(n), randn(n), randn(n)
    else:
        raise ValueError(c.op)
    return d


def contraction(c, d):
    """(M, v, k): the case's sum is M v (v = None: the column sums of M, no products), k terms per entry."""
    if c.op == "gemv_n":
        return d["A"], d["x"], c.cols
    if c.op == "gemv_t":
        return d["A"].T, d["x"], c.rows
    if c.op in ("symv", "symv_packed"):
        return d["A"], d["x"], c.rows
    return d["A"].T, None, c.nparts


def reference(c, d, dtype):
    """(reference, tolerance): the fp64 result on the rounded inputs and the forward bound per entry
    (a pair of floats for the reductions)."""
    if c.op in ("sumsq", "sumsq_diff", "dot"):
        if c.op == "sumsq":
            terms = d["x"] * d["x"]
        elif c.op == "sumsq_diff":
            terms = (d["x"] - d["y"]) ** 2
        else:
            terms = d["x"] * d["y"]
        start = PRESET if c.acc else 0.0
        ref = math.fsum([start] + terms.tolist())
        return ref, gamma(c.rows + 8, U["f64"]) * (abs(start) + math.fsum(np.abs(terms).tolist()))
    y = d["y"]
    by, aby = (c.beta * y, abs(c.beta) * np.abs(y)) if c.beta != 0 else (0.0, 0.0)
    if c.op in ("axpby", "diag_mul"):
        # in extended precision: at f64 an fp64 reference's own two or three roundings, in an order
        # of its own, would be as large as the bound on the kernel's three
        ext = np.longdouble
        t = ext(c.alpha) * d["x"].astype(ext)
        if c.op == "diag_mul":
            t = t * d["A"].astype(ext)
        ref = t + ext(c.beta) * y.astype(ext) if c.beta != 0 else t
        return ref, 4 * U[dtype] * (np.abs(t).astype(np.float64) + aby)
    M, v, k = contraction(c, d)
    if v is None:
        s, mag = M.sum(axis=1), np.abs(M).sum(axis=1)
    else:
        s, mag = M.dot(v), np.abs(M).dot(np.abs(v))
    ref = c.alpha * s + by
    mag = abs(c.alpha) * mag + aby
    if c.add:
        ref = ref + d["add"]
        mag = mag + np.abs(d["add"])
    return ref, gamma(k + 8, U[dtype]) * mag


def device_operands(c, d):
    """The keyword arguments of dense_op for case c: the operands as the device gets them - NaN in
    everything the launcher must not read (y under beta == 0, the padding rows of the matrix, the
    tiles of a symmetric matrix strictly above the block diagonal)."""
    kw = dict(rows=c.rows, cols=c.cols, alpha=c.alpha, beta=c.beta, nparts=c.nparts, use_work=c.work,
              accumulate=c.acc, alias_xy=c.alias, preset=PRESET,
              a_off=c.off[0], x_off=c.off[1], y_off=c.off[2], add_off=c.off[3])
    reduction = c.op in ("sumsq", "sumsq_diff", "dot")
    if "y" in d:
        nan_y = c.beta == 0 and not reduction and not c.alias
        kw["y"] = np.full(d["y"].shape, np.nan) if nan_y else d["y"]
    if "x" in d and not c.alias:
        kw["x"] = d["x"]
    if "add" in d:
        kw["add"] = d["add"]
    if c.op in ("gemv_n", "gemv_t", "symv", "symv_packed"):
        A = d["A"]
        rows, cols = A.shape
        lda = rows + c.pad
        kw["lda"] = lda
        P = np.full((lda, cols), np.nan)
        P[:rows] = A
        if c.op.startswith("symv"):
            blk = np.arange(rows) // SB
            P[:rows][blk[:, None] < blk[None, :]] = np.nan
        kw["a"] = P.flatten(order="F")[:(cols - 1) * lda + rows if cols else 0]
    elif "A" in d:
        kw["a"] = d["A"].reshape(-1)  # partials one after the other / the diagonal
    return kw


# ---- the checks -------------------------------------------------------------------------------------

@pytest.fixture(params=["f64", "f32"])
def dtype(request, solve_mod):
    solve_mod.set_option("dtype", request.param)
    yield request.param
    solve_mod.set_option("dtype", "f32")


def split_guards(c, out):
    assert out.shape == (len(out),) and len(out) >= 2 * G
    lo, body, hi = out[:G], out[G:len(out) - G], out[len(out) - G:]
    assert np.array_equal(lo, np.full(G, SENTINEL)), "%s: store below the output: %r" % (case_id(c), lo)
    assert np.array_equal(hi, np.full(G, SENTINEL)), "%s: store past the output: %r" % (case_id(c), hi)
    return body


def check_vector(c, got, ref, tol):
    assert np.all(np.isfinite(got)), "%s (%s): %d entries not finite (something that must not be read was)" % (
        case_id(c), c.note, np.count_nonzero(~np.isfinite(got)))
    err = np.abs(got - ref)
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, "%s (%s): %d entries outside the bound, first at %d: got %r, reference %r, bound %r" % (
        case_id(c), c.note, bad.size, bad[0], got[bad[0]], np.broadcast_to(ref, got.shape)[bad[0]],
        np.broadcast_to(tol, got.shape)[bad[0]])


def run_case(solve_mod, c, dtype):
    d = make_data(c, dtype)
    ref, tol = reference(c, d, dtype)
    kw = device_operands(c, d)
    first = solve_mod.dense_op(c.op, **kw)
    again = solve_mod.dense_op(c.op, **kw)
    if c.op in ("sumsq", "sumsq_diff", "dot"):
        assert math.isfinite(first)
        assert abs(first - ref) <= tol, "%s (%s): got %r, reference %r, bound %r" % (case_id(c), c.note, first, ref, tol)
        assert first == again, "%s: two runs differ: %r, %r" % (case_id(c), first, again)
        return first
    if c.op == "symv_packed":
        packed, plain = (split_guards(c, o) for o in first)
        check_vector(c, plain, ref, tol)
        check_vector(c, packed, ref, tol)
        assert np.array_equal(packed, plain), "%s: the packed apply differs from Symv in %d entries" % (
            case_id(c), np.count_nonzero(packed != plain))
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), "two runs differ"
        return packed
    got = split_guards(c, first)
    check_vector(c, got, ref, tol)
    assert np.array_equal(first, again), "%s (%s): two runs differ in %d entries" % (
        case_id(c), c.note, np.count_nonzero(first != again))
    return got


def params(cases):
    return pytest.mark.parametrize("c", cases, ids=[case_id(c) for c in cases])


@params(GEMV_N_CASES)
def test_gemv_n(solve_mod, dtype, c):
    run_case(solve_mod, c, dtype)


@params(GEMV_T_CASES)
def test_gemv_t(solve_mod, dtype, c):
    run_case(solve_mod, c, dtype)


@params(SYMV_CASES)
def test_symv(solve_mod, dtype, c):
    run_case(solve_mod, c, dtype)


@params(SYMV_PACKED_CASES)
def test_symv_packed_equals_symv(solve_mod, dtype, c):
    run_case(solve_mod, c, dtype)


@params(RP_CASES)
def test_reduce_partials(solve_mod, dtype, c):
    run_case(solve_mod, c, dtype)


@pytest.mark.parametrize("shape", RP_ALIGN_SHAPES, ids=["%dx%d" % s for s in RP_ALIGN_SHAPES])
def test_reduce_partials_unaligned_operand_agrees_with_float4_form(solve_mod, dtype, shape):
    """The float4 shapes with partial, y or add one element off 16-byte alignment fall back to the
    generic form: each result is inside the bound of the reference, so any two of them differ by at
    most twice the bound."""
    rows, nparts = shape
    group = [c for c in RP_ALIGN_CASES if (c.rows, c.nparts) == shape]
    assert len(group) == 4 and not any(group[0].off)
    base = group[0]
    d = make_data(base, dtype)  # one set of operands for the four placements
    ref, tol = reference(base, d, dtype)
    aligned = run_case(solve_mod, base, dtype)
    for c in group[1:]:
        kw = device_operands(c, d)
        first = solve_mod.dense_op(c.op, **kw)
        got = split_guards(c, first)
        check_vector(c, got, ref, tol)
        assert np.all(np.abs(got - aligned) <= 2 * tol), "%s disagrees with the aligned form" % case_id(c)
        assert np.array_equal(first, solve_mod.dense_op(c.op, **kw)), "%s: two runs differ" % case_id(c)


@params(RED_CASES)
def test_reductions(solve_mod, dtype, c):
    got = run_case(solve_mod, c, dtype)
    if c.rows == 0:
        assert got == (PRESET if c.acc else 0.0)


@params(AXPBY_CASES)
def test_axpby(solve_mod, dtype, c):
    run_case(solve_mod, c, dtype)


@params(DIAG_MUL_CASES)
def test_diag_mul(solve_mod, dtype, c):
    run_case(solve_mod, c, dtype)


def test_empty_contraction_is_exact(solve_mod, dtype):
    """Gemv on a matrix without columns (rows for the transpose): exactly 0, or exactly beta y for a
    beta that scales without rounding."""
    for c in GEMV_N_CASES[-2:] + GEMV_T_CASES[-2:]:
        assert c.rows * c.cols == 0
        d = make_data(c, dtype)
        got = run_case(solve_mod, c, dtype)
        assert np.array_equal(got, c.beta * d["y"])
