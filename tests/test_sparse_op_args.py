"""The test entries of the sparse layer (include/epsilon_hip.h eps_test_sparse_op, eps_test_csc_op,
eps_test_sparse_handle_op): the argument checks.  They fail before any device work - no malformed
structure may reach a kernel - so they need the built library, not a GPU."""

import os

import numpy as np
import pytest
import scipy.sparse as sp

from epsilon_amd import _solve, ir


@pytest.fixture(scope="module")
def lib_built():
    if not os.path.exists(_solve.LIB_PATH):
        pytest.fail("libepsilon_hip.so is not built")
    return _solve


# S = [[1 0 2 0], [0 0 0 0], [0 3 4 5]] in CSR
PTR, IDX, VAL = [0, 2, 2, 5], [0, 2, 1, 2, 3], [1.0, 2.0, 3.0, 4.0, 5.0]
X4, Y3 = np.ones(4), np.ones(3)


def spmv(**kw):
    args = dict(rows=3, cols=4, ptr=PTR, idx=IDX, val=VAL, d=X4, y=Y3)
    args.update(kw)
    return _solve.sparse_op(args.pop("op", "spmv"), **args)


def spmm(**kw):  # B is 4 x 2
    args = dict(op="spmm_csr_dense", d=np.ones(8), ld=4, n=2, y=np.ones(6))
    args.update(kw)
    return spmv(**args)


@pytest.mark.parametrize("op", ["", "spmm", "SPMV", "spmv_csr"])
def test_unknown_op(lib_built, op):
    with pytest.raises(_solve.error, match="eps_test_sparse_op: op must be spmv, spmm_csr_dense, dense_spmm_csc or "
                                           "scatter_add_csc, got %s$" % op):
        spmv(op=op)


def test_null_op(lib_built):
    with pytest.raises(_solve.error, match="eps_test_sparse_op: op is null"):
        spmv(op=None)


@pytest.mark.parametrize("missing", ["ptr", "idx", "val", "d", "y"])
def test_null_arrays(lib_built, missing):
    with pytest.raises(_solve.error, match="eps_test_sparse_op: %s is null" % missing):
        spmv(**{missing: None, "nnz": 5})
    if missing in ("d", "y"):
        with pytest.raises(_solve.error, match="eps_test_sparse_op: %s is null" % missing):
            spmm(**{missing: None})


def test_negative_sizes(lib_built):
    with pytest.raises(_solve.error, match="eps_test_sparse_op: rows is negative: -3"):
        spmv(rows=-3)
    with pytest.raises(_solve.error, match="eps_test_sparse_op: cols is negative: -4"):
        spmv(cols=-4)
    with pytest.raises(_solve.error, match="eps_test_sparse_op: nnz is negative: -1"):
        spmv(nnz=-1)
    with pytest.raises(_solve.error, match="eps_test_sparse_op: n is negative: -2"):
        spmm(n=-2)


def test_row_pointers(lib_built):
    with pytest.raises(_solve.error, match="eps_test_sparse_op: ptr has 4 entries, rows \\+ 1 is 3"):
        spmv(rows=2, y=np.ones(2))
    with pytest.raises(_solve.error, match="eps_test_sparse_op: ptr\\[0\\] is 1, not 0"):
        spmv(ptr=[1, 2, 2, 5])
    with pytest.raises(_solve.error, match="eps_test_sparse_op: ptr is not monotone at 1: 3 > 2"):
        spmv(ptr=[0, 3, 2, 5])
    with pytest.raises(_solve.error, match="eps_test_sparse_op: ptr ends at 4, nnz is 5"):
        spmv(ptr=[0, 2, 2, 4])
    with pytest.raises(_solve.error, match="eps_test_sparse_op: ptr ends at 7, nnz is 5"):
        spmv(ptr=[0, 2, 2, 7])  # would index past idx and val
    with pytest.raises(_solve.error, match="eps_test_sparse_op: idx has 4 entries, nnz is 5"):
        spmv(idx=IDX[:4])
    with pytest.raises(_solve.error, match="eps_test_sparse_op: val has 5 entries, nnz is 4"):
        spmv(nnz=4, idx=IDX[:4])


@pytest.mark.parametrize("op", ["spmv", "spmm_csr_dense", "dense_spmm_csc", "scatter_add_csc"])
def test_column_index_out_of_range(lib_built, op):
    """What matters on a shared machine: an index outside [0, cols) would make the kernel read or write
    outside its operands."""
    kw = {"spmv": {}, "spmm_csr_dense": dict(d=np.ones(8), ld=4, n=2, y=np.ones(6)),
          "dense_spmm_csc": dict(d=np.ones(8), ld=2, n=2, y=np.ones(6)),
          "scatter_add_csc": dict(d=None, y=np.ones(12))}[op]
    with pytest.raises(_solve.error, match="eps_test_sparse_op: idx\\[4\\] = 4 is outside \\[0, 4\\)"):
        spmv(op=op, idx=[0, 2, 1, 2, 4], **kw)
    with pytest.raises(_solve.error, match="eps_test_sparse_op: idx\\[1\\] = -1 is outside \\[0, 4\\)"):
        spmv(op=op, idx=[0, -1, 1, 2, 3], **kw)


def test_ld_too_small(lib_built):
    with pytest.raises(_solve.error, match="eps_test_sparse_op: ld 3 < rows 4"):
        spmm(ld=3)  # B holds cols = 4 rows per column
    with pytest.raises(_solve.error, match="eps_test_sparse_op: ld 1 < rows 2"):
        spmv(op="dense_spmm_csc", d=np.ones(8), ld=1, n=2, y=np.ones(6))  # A holds n = 2 rows per column


def test_operand_lengths(lib_built):
    with pytest.raises(_solve.error, match="d has 3 entries, the dimensions need 4"):
        spmv(d=np.ones(3))
    with pytest.raises(_solve.error, match="y has 4 entries, the dimensions need 3"):
        spmv(y=np.ones(4))
    with pytest.raises(_solve.error, match="d has 8 entries, the dimensions need 10"):
        spmm(ld=6)  # (n - 1) ld + cols
    with pytest.raises(_solve.error, match="y has 5 entries, the dimensions need 6"):
        spmm(y=np.ones(5))
    with pytest.raises(_solve.error, match="d has 8 entries, the dimensions need 11"):
        spmv(op="dense_spmm_csc", d=np.ones(8), ld=3, n=2, y=np.ones(6))  # (cols - 1) ld + n
    with pytest.raises(_solve.error, match="y has 3 entries, the dimensions need 12"):
        spmv(op="scatter_add_csc", d=None)  # W is cols x rows


def test_arguments_an_op_has_no_use_for(lib_built):
    with pytest.raises(_solve.error, match="eps_test_sparse_op: beta is given \\(0.5\\), spmm_csr_dense has none"):
        spmm(beta=0.5)
    with pytest.raises(_solve.error, match="eps_test_sparse_op: n is given \\(2\\), spmv has none"):
        spmv(n=2)
    with pytest.raises(_solve.error, match="eps_test_sparse_op: ld is given \\(4\\), spmv has none"):
        spmv(ld=4)
    with pytest.raises(_solve.error, match="eps_test_sparse_op: d is given, scatter_add_csc has none"):
        spmv(op="scatter_add_csc", y=np.ones(12))


def test_every_check_comes_before_device_work(lib_built):
    """With arguments that pass, the call goes on to the device: without one it fails there (no
    fallback), with one it answers."""
    calls = [dict(), dict(op="spmm_csr_dense", d=np.ones(8), ld=4, n=2, y=np.ones(6)),
             dict(op="dense_spmm_csc", d=np.ones(8), ld=2, n=2, y=np.ones(6)),
             dict(op="scatter_add_csc", d=None, y=np.ones(12))]
    if _solve.device_count() > 0:
        out = spmv()
        G = _solve.DENSE_OP_GUARD
        assert np.array_equal(out[G:-G], [3.0, 0.0, 12.0])
        assert np.all(out[:G] == _solve.DENSE_OP_SENTINEL) and np.all(out[-G:] == _solve.DENSE_OP_SENTINEL)
    else:
        for kw in calls:
            with pytest.raises(_solve.error, match="no HIP device"):
                spmv(**kw)


# ---- eps_test_csc_op: the host algebra, no device at all ----------------------------------------------

# A = [[1 0], [0 2], [3 4]] in CSC
A32 = (3, 2, [0, 2, 4], [0, 2, 1, 2], [1.0, 3.0, 2.0, 4.0])


def operand(base=A32, **kw):
    f = dict(zip(("m", "n", "colptr", "rowidx", "val"), base))
    f.update(kw)
    t = (f["m"], f["n"], f["colptr"], f["rowidx"], f["val"])
    return t + (f["nnz"],) if "nnz" in f else t


@pytest.mark.parametrize("op", ["", "mul", "TRANSPOSE", "from_csr"])
def test_csc_unknown_op(lib_built, op):
    with pytest.raises(_solve.error, match="eps_test_csc_op: op must be transpose, add, multiply, kron, scale_rows, "
                                           "scale_cols, from_dense or from_blob, got %s$" % op):
        _solve.csc_op(op, a=A32)


def test_csc_null_op_and_arrays(lib_built):
    with pytest.raises(_solve.error, match="eps_test_csc_op: op is null"):
        _solve.csc_op(None, a=A32)
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.colptr is null"):
        _solve.csc_op("transpose", a=operand(colptr=None))
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.rowidx is null"):
        _solve.csc_op("transpose", a=operand(rowidx=None, nnz=4))
    with pytest.raises(_solve.error, match="eps_test_csc_op: val is null"):
        _solve.csc_op("transpose", a=operand(val=None, nnz=4))
    with pytest.raises(_solve.error, match="eps_test_csc_op: b.colptr is null"):
        _solve.csc_op("add", a=A32, b=operand(colptr=None))
    with pytest.raises(_solve.error, match="eps_test_csc_op: d is null"):
        _solve.csc_op("scale_rows", a=A32)
    with pytest.raises(_solve.error, match="eps_test_csc_op: d is null"):
        _solve.csc_op("from_dense", m=2, n=2)
    with pytest.raises(_solve.error, match="eps_test_csc_op: blob is null"):
        _solve.csc_op("from_blob", m=2, n=2, nnz=1)


def test_csc_negative_sizes(lib_built):
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.m is negative: -3"):
        _solve.csc_op("transpose", a=operand(m=-3))
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.n is negative: -2"):
        _solve.csc_op("transpose", a=operand(n=-2), colptr_cap=4)
    with pytest.raises(_solve.error, match="eps_test_csc_op: nnz is negative: -1"):
        _solve.csc_op("transpose", a=operand(nnz=-1))
    with pytest.raises(_solve.error, match="eps_test_csc_op: b.m is negative: -3"):
        _solve.csc_op("add", a=A32, b=operand(m=-3))
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.m is negative: -1"):
        _solve.csc_op("from_dense", m=-1, n=2, d=np.ones(2))
    with pytest.raises(_solve.error, match="eps_test_csc_op: nnz is negative: -1"):
        _solve.csc_op("from_blob", m=2, n=2, nnz=-1, blob=b"x")
    with pytest.raises(_solve.error, match="eps_test_csc_op: colptr_cap is negative: -1"):
        _solve.csc_op("transpose", a=A32, colptr_cap=-1)
    with pytest.raises(_solve.error, match="eps_test_csc_op: nnz_cap is negative: -1"):
        _solve.csc_op("transpose", a=A32, nnz_cap=-1)


def test_csc_column_pointers_and_indices(lib_built):
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.colptr has 3 entries, a.n \\+ 1 is 4"):
        _solve.csc_op("transpose", a=operand(n=3))
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.colptr\\[0\\] is 1, not 0"):
        _solve.csc_op("transpose", a=operand(colptr=[1, 2, 4]))
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.colptr is not monotone at 1: 3 > 2"):
        _solve.csc_op("transpose", a=operand(colptr=[0, 3, 2, 4], n=3))
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.colptr ends at 3, nnz is 4"):
        _solve.csc_op("transpose", a=operand(colptr=[0, 2, 3]))
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.rowidx has 3 entries, nnz is 4"):
        _solve.csc_op("transpose", a=operand(rowidx=[0, 2, 1]))
    with pytest.raises(_solve.error, match="eps_test_csc_op: val has 3 entries, nnz is 4"):
        _solve.csc_op("transpose", a=operand(val=[1.0, 2.0, 3.0], nnz=4))
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.rowidx\\[3\\] = 3 is outside \\[0, 3\\)"):
        _solve.csc_op("transpose", a=operand(rowidx=[0, 2, 1, 3]))
    with pytest.raises(_solve.error, match="eps_test_csc_op: b.rowidx\\[0\\] = -1 is outside \\[0, 3\\)"):
        _solve.csc_op("add", a=A32, b=operand(rowidx=[-1, 2, 1, 2]))
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.rowidx is not strictly ascending at 1"):
        _solve.csc_op("transpose", a=operand(rowidx=[2, 0, 1, 2]))
    with pytest.raises(_solve.error, match="eps_test_csc_op: a.rowidx is not strictly ascending at 3"):
        _solve.csc_op("transpose", a=operand(rowidx=[0, 2, 1, 1]))


def test_csc_operands_that_do_not_fit(lib_built):
    B23 = (2, 3, [0, 1, 1, 2], [0, 1], [1.0, 1.0])
    with pytest.raises(_solve.error, match="eps_test_csc_op: add: a is 3 x 2, b is 2 x 3"):
        _solve.csc_op("add", a=A32, b=B23)
    with pytest.raises(_solve.error, match="eps_test_csc_op: multiply: a has 2 columns, b has 3 rows"):
        _solve.csc_op("multiply", a=A32, b=A32)
    with pytest.raises(_solve.error, match="eps_test_csc_op: d has 2 entries, scale_rows needs 1 or 3"):
        _solve.csc_op("scale_rows", a=A32, d=np.ones(2))
    with pytest.raises(_solve.error, match="eps_test_csc_op: d has 3 entries, scale_cols needs 1 or 2"):
        _solve.csc_op("scale_cols", a=A32, d=np.ones(3))
    with pytest.raises(_solve.error, match="eps_test_csc_op: d has 5 entries, the dimensions need 6"):
        _solve.csc_op("from_dense", m=3, n=2, d=np.ones(5))


def test_csc_result_capacities(lib_built):
    with pytest.raises(_solve.error, match="eps_test_csc_op: colptr_cap 3 < n \\+ 1 = 4"):
        _solve.csc_op("transpose", a=A32, colptr_cap=3)
    with pytest.raises(_solve.error, match="eps_test_csc_op: nnz_cap 3 < nnz = 4"):
        _solve.csc_op("transpose", a=A32, nnz_cap=3)


# ---- eps_test_sparse_handle_op ------------------------------------------------------------------------

S34 = ir.sparse_matrix(sp.csc_matrix(np.array([[1.0, 0, 2, 0], [0, 0, 0, 0], [0, 3, 4, 5]])))


def test_handle_op_arguments(lib_built):
    fn = "eps_test_sparse_handle_op: "
    with pytest.raises(_solve.error, match=fn + "op is null"):
        _solve.sparse_handle_op(None, S34, X4)
    with pytest.raises(_solve.error, match=fn + "op must be apply, adjoint, sparse_dense, dense_sparse, "
                                                "sparse_plus_dense or dense_plus_sparse, got multiply$"):
        _solve.sparse_handle_op("multiply", S34, X4)
    with pytest.raises(_solve.error, match=fn + "sparse_map is null or empty"):
        _solve.sparse_handle_op("apply", None, X4)
    with pytest.raises(_solve.error, match=fn + "d is null"):
        _solve.sparse_handle_op("apply", S34, None)
    with pytest.raises(_solve.error, match=fn + "sparse_map is not a sparse matrix: type 4"):
        _solve.sparse_handle_op("apply", ir.scalar(2.0, 4), X4)
    with pytest.raises(_solve.error, match=fn + "d is 3 x 1, apply with a 3 x 4 handle needs 4 x 1"):
        _solve.sparse_handle_op("apply", S34, Y3)
    with pytest.raises(_solve.error, match=fn + "d is 4 x 1, apply with a 4 x 3 handle needs 3 x 1"):
        _solve.sparse_handle_op("apply", S34, X4, transpose=True)
    with pytest.raises(_solve.error, match=fn + "d is 3 x 2, sparse_dense with a 3 x 4 handle needs 4 x 2"):
        _solve.sparse_handle_op("sparse_dense", S34, np.ones((3, 2)))
    with pytest.raises(_solve.error, match=fn + "d is 2 x 4, dense_sparse with a 3 x 4 handle needs 2 x 3"):
        _solve.sparse_handle_op("dense_sparse", S34, np.ones((2, 4)))
    with pytest.raises(_solve.error, match=fn + "d is 4 x 3, dense_plus_sparse with a 3 x 4 handle needs 3 x 4"):
        _solve.sparse_handle_op("dense_plus_sparse", S34, np.ones((4, 3)))
    with pytest.raises(_solve.error, match=fn + "p has 3 entries, the map has 4 columns"):
        _solve.sparse_handle_op("apply", S34, X4, p=Y3)
    if _solve.device_count() == 0:
        with pytest.raises(_solve.error, match="no HIP device"):
            _solve.sparse_handle_op("apply", S34, X4)
