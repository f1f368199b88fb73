"""ctypes binding of libepsilon_hip.so with the call signatures of `epopt._solve`.

Reference module: python/epopt/solvemodule.cc:265-271

    solve(problem_bytes, parameters, solver_params_bytes, data) -> (status_bytes, {var_id: bytes})
    eval_prox(f_expr_bytes, lam, data, v) -> {var_id: bytes}

`data` / `v` are {str: bytes}; values come back as float64 column-major bytes.  A failed
call raises `_solve.error`, as the reference does through its longjmp handler
(solvemodule.cc:245-248,286-289).  There is no fallback: if the library is not built or no
HIP device is present the call fails.
"""

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libepsilon_hip.so")


class error(Exception):
    """`_solve.error` (reference solvemodule.cc:286-289)."""


class _Blob(ctypes.Structure):
    _fields_ = [("key", ctypes.c_char_p), ("ptr", ctypes.c_void_p),
                ("len", ctypes.c_size_t), ("kind", ctypes.c_int)]


class _Param(ctypes.Structure):
    _fields_ = [("id", ctypes.c_char_p), ("constant_proto", ctypes.c_void_p),
                ("len", ctypes.c_size_t)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise error("libepsilon_hip.so is not built (run `python -m epsilon_amd.build`)")
        L = ctypes.CDLL(LIB_PATH)
        L.eps_last_error.restype = ctypes.c_char_p
        L.eps_version.restype = ctypes.c_char_p
        L.eps_result_num_vars.restype = ctypes.c_size_t
        L.eps_result_num_vars.argtypes = [ctypes.c_void_p]
        L.eps_result_free.argtypes = [ctypes.c_void_p]
        L.eps_result_copy_var.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        L.eps_result_copy_var.restype = ctypes.c_int
        L.eps_result_free.restype = None
        L.eps_solver_destroy.argtypes = [ctypes.c_void_p]
        L.eps_solver_destroy.restype = None
        L.eps_set_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise error(lib().eps_last_error().decode("utf-8", "replace") or "CHECK failed")


_options = {}  # what set_option last stored per key (solve_batch restores "batch_wide" from it)


def set_option(key, value):
    _check(lib().eps_set_option(key.encode(), str(value).encode()))
    _options[key] = str(value)


def device_count():
    return lib().eps_device_count()


def _blobs(d, keep):
    """{key: bytes | ("device", ptr, count, "f32"|"f64")} -> (array of eps_blob, n)."""
    items = list(d.items())
    arr = (_Blob * max(len(items), 1))()
    for i, (k, v) in enumerate(items):
        kb = k.encode("utf-8")
        keep.append(kb)
        arr[i].key = kb
        if isinstance(v, tuple) and v and v[0] == "device":
            arr[i].ptr = ctypes.c_void_p(v[1])
            arr[i].len = v[2]
            arr[i].kind = 1 if v[3] == "f32" else 2
        else:
            if isinstance(v, np.ndarray):
                v = np.ascontiguousarray(v)
                keep.append(v)
                arr[i].ptr = v.ctypes.data_as(ctypes.c_void_p)
                arr[i].len = v.nbytes
            elif isinstance(v, bytes):
                # the bytes object's own buffer (no copy: a data matrix can be gigabytes; the
                # library reads it during the call or copies what it keeps)
                keep.append(v)
                ref = ctypes.c_char_p(v) if len(v) else None
                keep.append(ref)
                arr[i].ptr = ctypes.cast(ref, ctypes.c_void_p) if ref is not None else None
                arr[i].len = len(v)
            else:
                buf = (ctypes.c_char * len(v)).from_buffer_copy(v) if len(v) else None
                keep.append(buf)
                arr[i].ptr = ctypes.cast(buf, ctypes.c_void_p) if buf is not None else None
                arr[i].len = len(v)
            arr[i].kind = 0
    return arr, len(items)


def _params(parameters, keep):
    items = list(parameters or [])
    arr = (_Param * max(len(items), 1))()
    for i, (pid, cbytes) in enumerate(items):
        pb = pid.encode("utf-8")
        buf = ctypes.create_string_buffer(cbytes, len(cbytes))
        keep.extend([pb, buf])
        arr[i].id = pb
        arr[i].constant_proto = ctypes.cast(buf, ctypes.c_void_p)
        arr[i].len = len(cbytes)
    return arr, len(items)


_BIG_RESULT = 64 << 20
_new_bytes = ctypes.pythonapi.PyBytes_FromStringAndSize
_new_bytes.restype = ctypes.py_object
_new_bytes.argtypes = [ctypes.c_void_p, ctypes.c_ssize_t]
_bytes_ptr = ctypes.pythonapi.PyBytes_AsString
_bytes_ptr.restype = ctypes.c_void_p
_bytes_ptr.argtypes = [ctypes.py_object]


def _take_result(res):
    L = lib()
    try:
        sp = ctypes.c_void_p()
        sl = ctypes.c_size_t()
        L.eps_result_status(res, ctypes.byref(sp), ctypes.byref(sl))
        status = ctypes.string_at(sp, sl.value) if sl.value else b""
        out = {}
        for i in range(L.eps_result_num_vars(res)):
            cid = ctypes.c_char_p()
            vals = ctypes.POINTER(ctypes.c_double)()
            cnt = ctypes.c_size_t()
            L.eps_result_var(res, ctypes.c_size_t(i), ctypes.byref(cid), ctypes.byref(vals),
                             ctypes.byref(cnt))
            nbytes = cnt.value * 8
            if nbytes >= _BIG_RESULT:
                # an uninitialised bytes object filled by the library's host threads before anyone
                # else sees it (the C-API contract of PyBytes_FromStringAndSize(NULL, n)); one
                # thread's string_at of a 0.8 GB iterate costs 0.15-0.2 s
                b = _new_bytes(None, nbytes)
                if L.eps_result_copy_var(res, ctypes.c_size_t(i), _bytes_ptr(b), ctypes.c_size_t(nbytes)) != 0:
                    raise error("eps_result_copy_var failed")
                out[cid.value.decode("utf-8")] = b
            else:
                out[cid.value.decode("utf-8")] = ctypes.string_at(vals, nbytes)
        return status, out
    finally:
        L.eps_result_free(res)


def solve(problem_bytes, parameters, solver_params_bytes, data):
    """reference `_solve.solve` (solvemodule.cc:110-187)."""
    L = lib()
    keep = []
    blobs, nb = _blobs(data, keep)
    params, np_ = _params(parameters, keep)
    res = ctypes.c_void_p()
    _check(L.eps_solve(problem_bytes, ctypes.c_size_t(len(problem_bytes)),
                       solver_params_bytes, ctypes.c_size_t(len(solver_params_bytes)),
                       blobs, ctypes.c_size_t(nb), params, ctypes.c_size_t(np_),
                       ctypes.byref(res)))
    return _take_result(res)


def solve_batch(problems, parameters, solver_params_bytes, data, wide=None):
    """K solves sharing `data` and the solver parameters (include/epsilon_hip.h eps_solve_batch):
    problems[k] with parameters[k] (a list of (id, constant_bytes) per instance, or None for
    none at all).  Returns [(status_bytes, {var_id: bytes})] in input order, each what `solve`
    returns for that instance alone.

    `wide`: None leaves the "batch_wide" option as it is; True / False set it for this call and
    restore the previous value afterwards.  Groups that run on the wide route match the single
    solve to f32 rounding, not bit for bit (eps_solve_batch in the header)."""
    if wide is None:
        return _solve_batch(problems, parameters, solver_params_bytes, data)
    previous = _options.get("batch_wide", os.environ.get("EPSILON_HIP_BATCH_WIDE", "0"))
    set_option("batch_wide", "1" if wide else "0")
    try:
        return _solve_batch(problems, parameters, solver_params_bytes, data)
    finally:
        set_option("batch_wide", previous)


def _solve_batch(problems, parameters, solver_params_bytes, data):
    L = lib()
    problems = list(problems)
    count = len(problems)
    if parameters is None:
        parameters = [[] for _ in problems]
    parameters = list(parameters)
    if len(parameters) != count:
        raise error("solve_batch: %d problems but %d parameter lists" % (count, len(parameters)))
    keep = []
    blobs, nb = _blobs(data, keep)
    n = max(count, 1)
    pbufs = (ctypes.c_void_p * n)()
    plens = (ctypes.c_size_t * n)()
    parr = (ctypes.c_void_p * n)()
    nparr = (ctypes.c_size_t * n)()
    for k, (pbytes, plist) in enumerate(zip(problems, parameters)):
        buf = ctypes.create_string_buffer(pbytes, len(pbytes))
        keep.append(buf)
        pbufs[k] = ctypes.cast(buf, ctypes.c_void_p)
        plens[k] = len(pbytes)
        arr, cnt = _params(plist, keep)
        keep.append(arr)
        parr[k] = ctypes.cast(arr, ctypes.c_void_p)
        nparr[k] = cnt
    res = (ctypes.c_void_p * n)()
    _check(L.eps_solve_batch(pbufs, plens, ctypes.c_size_t(count), solver_params_bytes,
                             ctypes.c_size_t(len(solver_params_bytes)), blobs, ctypes.c_size_t(nb),
                             parr, nparr, res))
    out = []
    try:
        for k in range(count):
            out.append(_take_result(ctypes.c_void_p(res[k])))
            res[k] = None
    finally:
        for k in range(count):
            if res[k]:
                L.eps_result_free(ctypes.c_void_p(res[k]))
    return out


def eval_prox(f_expr_bytes, lam, data, v):
    """reference `_solve.eval_prox` (solvemodule.cc:189-242)."""
    L = lib()
    keep = []
    blobs, nb = _blobs(data, keep)
    vb, nv = _blobs(v, keep)
    res = ctypes.c_void_p()
    _check(L.eps_eval_prox(f_expr_bytes, ctypes.c_size_t(len(f_expr_bytes)),
                           ctypes.c_double(lam), blobs, ctypes.c_size_t(nb), vb,
                           ctypes.c_size_t(nv), ctypes.byref(res)))
    return _take_result(res)[1]


class Solver(object):
    """Live solver handle (include/epsilon_hip.h eps_solver_*): keeps the data matrix, the
    cached factorisation and the iterates in HBM between calls (warm start; staged timing)."""

    def __init__(self, problem_bytes, solver_params_bytes, data):
        L = lib()
        keep = []  # host blobs are copied by the library: nothing to keep alive after the call
        blobs, nb = _blobs(data, keep)
        self._h = ctypes.c_void_p()
        _check(L.eps_solver_create(problem_bytes, ctypes.c_size_t(len(problem_bytes)),
                                   solver_params_bytes,
                                   ctypes.c_size_t(len(solver_params_bytes)), blobs,
                                   ctypes.c_size_t(nb), ctypes.byref(self._h)))

    def set_parameter(self, parameter_id, constant_bytes, data=None):
        keep = []
        blobs, nb = _blobs(data or {}, keep)
        _check(lib().eps_solver_set_parameter(self._h, parameter_id.encode(), constant_bytes,
                                              ctypes.c_size_t(len(constant_bytes)), blobs,
                                              ctypes.c_size_t(nb)))

    def init(self):
        _check(lib().eps_solver_init(self._h))

    def run(self, max_sweeps=-1):
        done = ctypes.c_int()
        _check(lib().eps_solver_run(self._h, ctypes.c_int(max_sweeps), ctypes.byref(done)))
        return done.value

    def result(self):
        res = ctypes.c_void_p()
        _check(lib().eps_solver_result(self._h, ctypes.byref(res)))
        return _take_result(res)

    def timing(self):
        a, b = ctypes.c_double(), ctypes.c_double()
        lib().eps_solver_timing(self._h, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def close(self):
        if self._h:
            lib().eps_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- sharded solves ---------------------------------------------------------------------------------

ALLREDUCE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                ctypes.c_void_p)
_comm_keep = []


def comm_unique_id():
    buf = ctypes.create_string_buffer(128)
    _check(lib().eps_comm_unique_id(buf))
    return buf.raw


def comm_init_rccl(rank, world, unique_id):
    _check(lib().eps_comm_init_rccl(ctypes.c_int(rank), ctypes.c_int(world), unique_id))


def comm_init_callback(rank, world, fn):
    """fn(numpy_array) must sum the array in place across ranks."""
    def trampoline(ptr, count, dtype, ctx):
        ctype = ctypes.c_float if dtype == 0 else ctypes.c_double
        arr = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(count,))
        fn(arr)
    cb = ALLREDUCE_FN(trampoline)
    _comm_keep.append(cb)
    _check(lib().eps_comm_init_callback(ctypes.c_int(rank), ctypes.c_int(world), cb, None))


def comm_warmup(count=1 << 20):
    """Collective: one checked all-reduce + all-gather of `count` floats (barrier + RCCL first-use
    setup)."""
    _check(lib().eps_comm_warmup(ctypes.c_size_t(count)))


def comm_enable_peer(slot_floats=0, rehearse_ranks=0):
    """Collective: set up the one-shot peer-write window (include/epsilon_hip.h).  Returns
    (enabled, reason-if-not)."""
    on = ctypes.c_int(0)
    _check(lib().eps_comm_enable_peer(ctypes.c_size_t(slot_floats), ctypes.c_int(rehearse_ranks),
                                      ctypes.byref(on)))
    return bool(on.value), ("" if on.value else lib().eps_last_error().decode("utf-8", "replace"))


def comm_disable_peer():
    _check(lib().eps_comm_disable_peer())


def comm_shutdown():
    _check(lib().eps_comm_shutdown())
    del _comm_keep[:]


def shard_keys(keys):
    keys = [k.encode("utf-8") for k in keys]
    arr = (ctypes.c_char_p * max(len(keys), 1))(*keys)
    _check(lib().eps_shard_keys(arr, ctypes.c_size_t(len(keys))))


def shard_consensus_terms(on=True):
    _check(lib().eps_shard_consensus_terms(ctypes.c_int(1 if on else 0)))


def block_solve_stats(reset=False):
    """(largest kappa_1 estimate of a pivot block, refinement steps) since the last reset (fp32)."""
    c, r = ctypes.c_double(0), ctypes.c_int(0)
    _check(lib().eps_block_solve_stats(ctypes.byref(c), ctypes.byref(r), ctypes.c_int(1 if reset else 0)))
    return c.value, r.value


def profile_enable(on=True):
    _check(lib().eps_profile_enable(ctypes.c_int(1 if on else 0)))


def profile_reset():
    _check(lib().eps_profile_reset())


def profile_dump():
    """{tag: (count, total_ms)} of the live HIP-event kernel timers."""
    buf = ctypes.create_string_buffer(1 << 16)
    _check(lib().eps_profile_dump(buf, ctypes.c_size_t(len(buf))))
    out = {}
    for line in buf.value.decode().splitlines():
        tag, count, ms = line.rsplit(" ", 2)
        out[tag] = (int(count), float(ms))
    return out


# ---- per-operator entry points ------------------------------------------------------------------


def linear_map_apply(lmap, x, transpose=False, inverse=False):
    """y = A x (or A^T x, or A^-1 x through the explicit inverse map) for an `ir.LMap`."""
    L = lib()
    keep = []
    blobs, nb = _blobs(lmap.data, keep)
    pbytes = lmap.proto.SerializeToString()
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    ny = lmap.n if transpose else lmap.m
    y = np.empty(ny, dtype=np.float64)
    _check(L.eps_linear_map_apply(pbytes, ctypes.c_size_t(len(pbytes)), blobs,
                                  ctypes.c_size_t(nb),
                                  ctypes.c_int((1 if transpose else 0) | (2 if inverse else 0)),
                                  x.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(x.size),
                                  y.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(ny)))
    return y


def linear_map_binary(op, A, B, ta=False, tb=False):
    """(result ImplType, dense m x n values) of A op B through the dispatch tables."""
    L = lib()
    keep = []
    data = dict(A.data)
    data.update(B.data)
    blobs, nb = _blobs(data, keep)
    ab, bb = A.proto.SerializeToString(), B.proto.SerializeToString()
    am, an = (A.n, A.m) if ta else (A.m, A.n)
    bm, bn = (B.n, B.m) if tb else (B.m, B.n)
    m, n = (am, an) if op == "+" else (am, bn)
    dense = np.empty(m * n, dtype=np.float64)
    rt = ctypes.c_int()
    mm, nn = ctypes.c_int64(), ctypes.c_int64()
    _check(L.eps_linear_map_binary(ctypes.c_char(op.encode()), ab, ctypes.c_size_t(len(ab)),
                                   ctypes.c_int(int(ta)), bb, ctypes.c_size_t(len(bb)),
                                   ctypes.c_int(int(tb)), blobs, ctypes.c_size_t(nb),
                                   ctypes.byref(rt), ctypes.byref(mm), ctypes.byref(nn),
                                   dense.ctypes.data_as(ctypes.c_void_p),
                                   ctypes.c_size_t(dense.size)))
    return rt.value, dense.reshape((mm.value, nn.value), order="F")


def linear_map_inverse(A):
    L = lib()
    keep = []
    blobs, nb = _blobs(A.data, keep)
    ab = A.proto.SerializeToString()
    dense = np.empty(A.m * A.n, dtype=np.float64)
    _check(L.eps_linear_map_inverse(ab, ctypes.c_size_t(len(ab)), blobs, ctypes.c_size_t(nb),
                                    dense.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.c_size_t(dense.size)))
    return dense.reshape((A.n, A.m), order="F")


class _Block(ctypes.Structure):
    _fields_ = [("row", ctypes.c_char_p), ("col", ctypes.c_char_p),
                ("linear_map", ctypes.c_void_p), ("len", ctypes.c_size_t)]


FILL_MAX = -1  # block_solve's fill bound of a key without a diagonal block


def block_solve(blocks, rhs=None, mode="factor", keys=None):
    """Test entry for the block LDL^T (include/epsilon_hip.h eps_test_block_solve).

    blocks: [(row key, col key, ir.LMap)] - both triangles of the symmetric matrix (for the modes
    "forward" / "back": the blocks of L / L^T); rhs: {key: float64 values}; keys: the substitution
    order of "forward" / "back".  Returns a dict with the entries the mode produces:

      "fill"                {key: bound}                          ("fill"; FILL_MAX: no diagonal block)
      "trace"               [({key: bound}, pivot)] per step      ("factor", "solve")
      "order"               [key]
      "L", "D_inv"          {(row, col): (ImplType, m x n array)}  ("factor"; a Kronecker product
                            has (4, ImplType of A, ImplType of B) in place of the ImplType)
      "condition_estimate", "refine_steps"
      "x", "x_again"        {key: array}    Solve(rhs) twice on the one factorisation; for
                                            "forward" / "back" "x" is the substituted vector
    """
    L = lib()
    keep = []
    blocks = list(blocks) if blocks is not None else None
    data = {}
    if blocks is None:
        barr, nblocks = None, 0
    else:
        nblocks = len(blocks)
        barr = (_Block * max(nblocks, 1))()
        for i, (row, col, lmap) in enumerate(blocks):
            rb, cb = row.encode("utf-8"), col.encode("utf-8")
            if isinstance(lmap, (bytes, bytearray)):
                payload = bytes(lmap)
            else:
                payload = lmap.proto.SerializeToString()
                data.update(lmap.data)
            buf = ctypes.create_string_buffer(payload, max(len(payload), 1))
            keep.extend([rb, cb, buf])
            barr[i].row, barr[i].col = rb, cb
            barr[i].linear_map = ctypes.cast(buf, ctypes.c_void_p)
            barr[i].len = len(payload)
    dblobs, nd = _blobs(data, keep)
    rblobs, nr = _blobs({k: np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
                         for k, v in (rhs or {}).items()}, keep)
    kb = [k.encode("utf-8") for k in (keys or [])]
    karr = (ctypes.c_char_p * max(len(kb), 1))(*kb)
    res = ctypes.c_void_p()
    _check(L.eps_test_block_solve(mode.encode("utf-8"), barr, ctypes.c_size_t(nblocks), dblobs,
                                  ctypes.c_size_t(nd), rblobs, ctypes.c_size_t(nr), karr,
                                  ctypes.c_size_t(len(kb)), ctypes.byref(res)))
    out = {}
    steps = {}
    order = {}
    for name, raw in _take_result(res)[1].items():
        f = name.split("\t")
        v = np.frombuffer(raw, dtype=np.float64)
        if f[0] == "fill":
            out.setdefault("fill", {})[f[1]] = int(v[0])
        elif f[0] == "trace":
            steps.setdefault(int(f[1]), [{}, None])[0][f[2]] = int(v[0])
        elif f[0] == "pivot":
            steps.setdefault(int(f[1]), [{}, None])[1] = f[2]
        elif f[0] == "order":
            order[int(f[1])] = f[2]
        elif f[0] in ("L", "D_inv"):
            m, n = int(v[1]), int(v[2])
            kind = int(v[0]) if v[3] < 0 else (int(v[0]), int(v[3]), int(v[4]))
            out.setdefault(f[0], {})[(f[1], f[2])] = (kind, v[5:].reshape((m, n), order="F").copy())
        elif f[0] in ("x", "x_again"):
            out.setdefault(f[0], {})[f[1]] = v.copy()
        elif f[0] == "refine_steps":
            out[f[0]] = int(v[0])
        else:
            out[f[0]] = float(v[0])
    if mode in ("factor", "solve"):
        out["trace"] = [tuple(steps[s]) for s in sorted(steps)]
        out["order"] = [order[i] for i in sorted(order)]
    return out


class _DenseOp(ctypes.Structure):
    _fields_ = [("op", ctypes.c_char_p),
                ("rows", ctypes.c_int64), ("cols", ctypes.c_int64), ("lda", ctypes.c_int64),
                ("nparts", ctypes.c_int), ("alpha", ctypes.c_double), ("beta", ctypes.c_double),
                ("a", ctypes.c_void_p), ("a_len", ctypes.c_int64), ("a_off", ctypes.c_int64),
                ("x", ctypes.c_void_p), ("x_len", ctypes.c_int64), ("x_off", ctypes.c_int64),
                ("y", ctypes.c_void_p), ("y_len", ctypes.c_int64), ("y_off", ctypes.c_int64),
                ("add", ctypes.c_void_p), ("add_len", ctypes.c_int64), ("add_off", ctypes.c_int64),
                ("accumulate", ctypes.c_int), ("use_work", ctypes.c_int), ("with_add", ctypes.c_int),
                ("alias_xy", ctypes.c_int), ("preset", ctypes.c_double)]


DENSE_OP_GUARD = 8            # EPS_DENSE_OP_GUARD
DENSE_OP_SENTINEL = -777.25   # EPS_DENSE_OP_SENTINEL
DENSE_OP_REDUCTIONS = ("sumsq", "sumsq_diff", "dot")


def _set_operands(g, operands):
    """Point the fields `name` and `name`_len of the struct g at each given (name, value) as
    contiguous float64; returns the arrays, which must outlive the call that reads g."""
    keep = []
    for name, v in operands:
        if v is not None:
            v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
            keep.append(v)
            setattr(g, name, v.ctypes.data_as(ctypes.c_void_p))
            setattr(g, name + "_len", v.size)
    return keep


def dense_op(op, rows=0, cols=0, lda=None, nparts=1, alpha=1.0, beta=0.0, a=None, x=None, y=None,
             add=None, a_off=0, x_off=0, y_off=0, add_off=0, accumulate=False, use_work=False,
             with_add=None, alias_xy=False, preset=0.0):
    """Test entry for the dense mat-vec layer (include/epsilon_hip.h eps_test_dense_op): one call
    of the launcher `op` names on the given float64 operands (a: the matrix, column-major with
    leading dimension lda, the partials, or the diagonal), each placed *_off elements into a
    larger device allocation.

    The reductions return the slot's value (it holds `preset` before the call).  The others return
    the output with its DENSE_OP_GUARD guard elements on each side (DENSE_OP_SENTINEL if nothing
    stored outside the output); "symv_packed" returns the pair (packed apply, plain Symv)."""
    L = lib()
    L.eps_test_dense_op.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    g = _DenseOp()
    g.op = op.encode("utf-8") if op is not None else None
    g.rows, g.cols, g.nparts = rows, cols, nparts
    g.lda = rows if lda is None else lda
    g.alpha, g.beta, g.preset = alpha, beta, preset
    keep = _set_operands(g, (("a", a), ("x", x), ("y", y), ("add", add)))
    g.a_off, g.x_off, g.y_off, g.add_off = a_off, x_off, y_off, add_off
    g.accumulate, g.use_work, g.alias_xy = int(accumulate), int(use_work), int(alias_xy)
    g.with_add = int(add is not None if with_add is None else with_add)
    n_out = 1 if op in DENSE_OP_REDUCTIONS else g.y_len + 2 * DENSE_OP_GUARD
    out = np.full(max(n_out, 1), np.nan)
    out2 = np.full(max(n_out, 1), np.nan) if op == "symv_packed" else None
    _check(L.eps_test_dense_op(ctypes.byref(g), out.ctypes.data_as(ctypes.c_void_p),
                               out2.ctypes.data_as(ctypes.c_void_p) if out2 is not None else None))
    if op in DENSE_OP_REDUCTIONS:
        return float(out[0])
    return (out[:n_out], out2[:n_out]) if out2 is not None else out[:n_out]


class _GemmOp(ctypes.Structure):
    _fields_ = [("op", ctypes.c_char_p), ("trans_a", ctypes.c_int), ("trans_b", ctypes.c_int),
                ("M", ctypes.c_int64), ("N", ctypes.c_int64), ("K", ctypes.c_int64),
                ("alpha", ctypes.c_double), ("beta", ctypes.c_double),
                ("lda", ctypes.c_int64), ("ldb", ctypes.c_int64), ("ldc", ctypes.c_int64),
                ("a_off", ctypes.c_int64), ("b_off", ctypes.c_int64), ("c_off", ctypes.c_int64),
                ("batch", ctypes.c_int64), ("outer", ctypes.c_int64), ("sA", ctypes.c_int64),
                ("sB", ctypes.c_int64), ("sC", ctypes.c_int64), ("sA2", ctypes.c_int64), ("sB2", ctypes.c_int64),
                ("lower_only", ctypes.c_int),
                ("a", ctypes.c_void_p), ("a_len", ctypes.c_int64), ("b", ctypes.c_void_p), ("b_len", ctypes.c_int64),
                ("c", ctypes.c_void_p), ("c_len", ctypes.c_int64), ("d", ctypes.c_void_p), ("d_len", ctypes.c_int64)]


def gemm_op(op, M=0, N=0, K=0, trans_a=False, trans_b=False, alpha=1.0, beta=0.0, lda=None, ldb=None,
            ldc=None, a=None, b=None, c=None, d=None, a_off=0, b_off=0, c_off=0, batch=1, outer=1,
            sA=0, sB=0, sC=0, sA2=0, sB2=0, lower_only=False):
    """Test entry for the dense mat-mat layer (include/epsilon_hip.h eps_test_gemm_op): one call of
    the launcher `op` names on float64 operands that are copied verbatim - the caller fills the
    padding rows of every column and the gaps between batch members - *_off elements into larger
    device allocations.  A leading dimension left None is the smallest that holds the operand.

    Returns (out, route): the whole result allocation with its DENSE_OP_GUARD guard elements on
    each side (DENSE_OP_SENTINEL if nothing stored there), and the branch Gemm took ("" for the
    helpers)."""
    L = lib()
    L.eps_test_gemm_op.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    g = _GemmOp()
    g.op = op.encode("utf-8") if op is not None else None
    g.trans_a, g.trans_b, g.lower_only = int(trans_a), int(trans_b), int(lower_only)
    g.M, g.N, g.K, g.alpha, g.beta = M, N, K, alpha, beta
    g.lda = ((N if op == "mat_copy" else K) if trans_a else M) if lda is None else lda
    g.ldb = (N if trans_b else K) if ldb is None else ldb
    g.ldc = M if ldc is None else ldc
    g.a_off, g.b_off, g.c_off = a_off, b_off, c_off
    g.batch, g.outer, g.sA, g.sB, g.sC, g.sA2, g.sB2 = batch, outer, sA, sB, sC, sA2, sB2
    keep = _set_operands(g, (("a", a), ("b", b), ("c", c), ("d", d)))
    n_out = (max(N, 0) if op == "col_abs_sums" else g.c_len) + 2 * DENSE_OP_GUARD
    out = np.full(n_out, np.nan)
    route = ctypes.create_string_buffer(32)
    _check(L.eps_test_gemm_op(ctypes.byref(g), out.ctypes.data_as(ctypes.c_void_p), route, ctypes.c_size_t(32)))
    return out, route.value.decode()


class _FactorOp(ctypes.Structure):
    _fields_ = [("op", ctypes.c_char_p), ("n", ctypes.c_int64), ("form", ctypes.c_int),
                ("a", ctypes.c_void_p), ("a_len", ctypes.c_int64), ("a_off", ctypes.c_int64),
                ("lo", ctypes.c_int64), ("cnt", ctypes.c_int64), ("out_cols", ctypes.c_int64)]


def factor_op(op, n=0, a=None, a_off=0, form=-1, lo=0, cnt=0, out_cols=None, want_out2=False):
    """Test entry for the dense factor layer (include/epsilon_hip.h eps_test_factor_op): one call of
    SpdInverseInPlace ("spd_inverse") or SpdInverseColumns ("spd_inverse_columns") on the n x n
    float64 matrix a (column-major, copied as given, upper triangle included), placed a_off
    elements into a larger device allocation, with the Cholesky step in `form`.

    Returns (out, out2).  out is the result between its DENSE_OP_GUARD guard elements
    (DENSE_OP_SENTINEL unless something stored there): the n * n inverse, or the n * out_cols slab
    (out_cols defaults to cnt) whose columns cnt .. out_cols must come back as the sentinel.  out2
    is None unless want_out2: X = L^-1 for "spd_inverse", W after the call - the Cholesky factor in
    its lower triangle - for "spd_inverse_columns"; n * n values."""
    L = lib()
    L.eps_test_factor_op.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    g = _FactorOp()
    g.op = op.encode("utf-8") if op is not None else None
    g.n, g.form, g.a_off, g.lo, g.cnt = n, form, a_off, lo, cnt
    g.out_cols = (cnt if op == "spd_inverse_columns" else 0) if out_cols is None else out_cols
    keep = _set_operands(g, (("a", a),))
    nn = max(n, 0) ** 2
    body = max(n, 0) * max(g.out_cols, 0) if op == "spd_inverse_columns" else nn
    out = np.full(body + 2 * DENSE_OP_GUARD, np.nan)
    out2 = np.full(nn, np.nan) if want_out2 else None
    _check(L.eps_test_factor_op(ctypes.byref(g), out.ctypes.data_as(ctypes.c_void_p),
                                out2.ctypes.data_as(ctypes.c_void_p) if out2 is not None else None))
    return out, out2


class _SparseOp(ctypes.Structure):
    _fields_ = [("op", ctypes.c_char_p),
                ("rows", ctypes.c_int64), ("cols", ctypes.c_int64), ("nnz", ctypes.c_int64),
                ("ptr", ctypes.c_void_p), ("ptr_len", ctypes.c_int64),
                ("idx", ctypes.c_void_p), ("idx_len", ctypes.c_int64),
                ("val", ctypes.c_void_p), ("val_len", ctypes.c_int64),
                ("alpha", ctypes.c_double), ("beta", ctypes.c_double),
                ("d", ctypes.c_void_p), ("d_len", ctypes.c_int64), ("ld", ctypes.c_int64), ("n", ctypes.c_int64),
                ("y", ctypes.c_void_p), ("y_len", ctypes.c_int64)]


def _set_indices(g, operands):
    """As _set_operands for int32 arrays."""
    keep = []
    for name, v in operands:
        if v is not None:
            v = np.ascontiguousarray(v, dtype=np.int32).reshape(-1)
            keep.append(v)
            setattr(g, name, v.ctypes.data_as(ctypes.c_void_p))
            setattr(g, name + "_len", v.size)
    return keep


def sparse_op(op, rows=0, cols=0, ptr=None, idx=None, val=None, nnz=None, alpha=1.0, beta=0.0, d=None,
              ld=0, n=0, y=None):
    """Test entry for the sparse layer (include/epsilon_hip.h eps_test_sparse_op): one call of the
    launcher `op` names ("spmv", "spmm_csr_dense", "dense_spmm_csc", "scatter_add_csc") on the CSR
    operand (ptr, idx, val), rows x cols, the dense operand d (copied verbatim, leading dimension
    ld, n columns of B / rows of A) and the initial output y.  nnz defaults to the length of val.

    Returns the output with its DENSE_OP_GUARD guard elements on each side (DENSE_OP_SENTINEL if
    nothing stored outside the output)."""
    L = lib()
    L.eps_test_sparse_op.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    g = _SparseOp()
    g.op = op.encode("utf-8") if op is not None else None
    g.rows, g.cols, g.alpha, g.beta, g.ld, g.n = rows, cols, alpha, beta, ld, n
    keep = _set_indices(g, (("ptr", ptr), ("idx", idx))) + _set_operands(g, (("val", val), ("d", d), ("y", y)))
    g.nnz = g.val_len if nnz is None else nnz
    out = np.full(g.y_len + 2 * DENSE_OP_GUARD, np.nan)
    _check(L.eps_test_sparse_op(ctypes.byref(g), out.ctypes.data_as(ctypes.c_void_p)))
    del keep
    return out


class _Csc(ctypes.Structure):
    _fields_ = [("m", ctypes.c_int64), ("n", ctypes.c_int64), ("nnz", ctypes.c_int64),
                ("colptr", ctypes.c_void_p), ("colptr_len", ctypes.c_int64),
                ("rowidx", ctypes.c_void_p), ("rowidx_len", ctypes.c_int64),
                ("val", ctypes.c_void_p), ("val_len", ctypes.c_int64)]


class _CscOp(ctypes.Structure):
    _fields_ = [("op", ctypes.c_char_p), ("a", _Csc), ("b", _Csc),
                ("d", ctypes.c_void_p), ("d_len", ctypes.c_int64),
                ("blob", ctypes.c_void_p), ("blob_len", ctypes.c_size_t),
                ("colptr", ctypes.c_void_p), ("colptr_cap", ctypes.c_int64),
                ("rowidx", ctypes.c_void_p), ("val", ctypes.c_void_p), ("nnz_cap", ctypes.c_int64)]


def _set_csc(c, operand, keep):
    """operand: (m, n, colptr, rowidx, val) or (m, n, colptr, rowidx, val, nnz); None entries stay null."""
    if operand is None:
        return 0
    c.m, c.n = operand[0], operand[1]
    keep += _set_indices(c, (("colptr", operand[2]), ("rowidx", operand[3])))
    keep += _set_operands(c, (("val", operand[4]),))
    c.nnz = operand[5] if len(operand) > 5 else c.val_len
    return c.nnz


def csc_op(op, a=None, b=None, d=None, blob=None, m=0, n=0, nnz=0, colptr_cap=None, nnz_cap=None):
    """Test entry for the host CSC algebra (include/epsilon_hip.h eps_test_csc_op; no device):
    "transpose", "add", "multiply", "kron", "scale_rows", "scale_cols" on the operands a and b, each
    (m, n, colptr, rowidx, val); "from_dense" on the column-major m x n values d; "from_blob" on
    the wire bytes `blob` of an m x n matrix with nnz entries.  The capacities of the result
    buffers default to what the op can produce at most.

    Returns (m, n, colptr, rowidx, val) of the result."""
    L = lib()
    L.eps_test_csc_op.argtypes = [ctypes.c_void_p] * 4
    g = _CscOp()
    g.op = op.encode("utf-8") if op is not None else None
    keep = []
    na, nb = _set_csc(g.a, a, keep), _set_csc(g.b, b, keep)
    if a is None:
        g.a.m, g.a.n, g.a.nnz = m, n, nnz
    keep += _set_operands(g, (("d", d),))
    if blob is not None:
        blob = bytes(blob)
        buf = ctypes.create_string_buffer(blob, max(len(blob), 1))
        keep.append(buf)
        g.blob, g.blob_len = ctypes.cast(buf, ctypes.c_void_p), len(blob)
    if colptr_cap is None:
        colptr_cap = max({"transpose": g.a.m, "add": g.a.n, "multiply": g.b.n, "kron": g.a.n * g.b.n}.get(op, g.a.n), 0) + 1
    if nnz_cap is None:
        nnz_cap = max({"add": na + nb, "multiply": g.a.m * g.b.n, "kron": na * nb, "from_dense": g.d_len,
                       "from_blob": nnz}.get(op, na), 0)
    colptr = np.zeros(max(colptr_cap, 1), dtype=np.int32)
    rowidx = np.zeros(max(nnz_cap, 1), dtype=np.int32)
    val = np.zeros(max(nnz_cap, 1), dtype=np.float64)
    g.colptr, g.colptr_cap = colptr.ctypes.data_as(ctypes.c_void_p), colptr_cap
    g.rowidx, g.val, g.nnz_cap = rowidx.ctypes.data_as(ctypes.c_void_p), val.ctypes.data_as(ctypes.c_void_p), nnz_cap
    rm, rn, rnnz = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _check(L.eps_test_csc_op(ctypes.byref(g), ctypes.byref(rm), ctypes.byref(rn), ctypes.byref(rnnz)))
    del keep
    return rm.value, rn.value, colptr[:rn.value + 1].copy(), rowidx[:rnnz.value].copy(), val[:rnnz.value].copy()


class _SparseHandleOp(ctypes.Structure):
    _fields_ = [("op", ctypes.c_char_p), ("sparse_map", ctypes.c_void_p), ("len", ctypes.c_size_t),
                ("data", ctypes.c_void_p), ("ndata", ctypes.c_size_t),
                ("transpose", ctypes.c_int), ("scaled", ctypes.c_int), ("scale", ctypes.c_double),
                ("p", ctypes.c_void_p), ("p_len", ctypes.c_int64),
                ("d", ctypes.c_void_p), ("d_rows", ctypes.c_int64), ("d_cols", ctypes.c_int64)]


def sparse_handle_op(op, S, d, transpose=False, scale=None, p=None):
    """Test entry for a sparse map handle as an operand (include/epsilon_hip.h
    eps_test_sparse_handle_op): the handle is the sparse ir.LMap S, transposed with `transpose`,
    then multiplied by the scalar map scale * I unless scale is None; `op` ("apply", "adjoint",
    "sparse_dense", "dense_sparse", "sparse_plus_dense", "dense_plus_sparse") combines it with the
    dense operand d (1-D for "apply" / "adjoint").  With p the map as built is applied to p first.

    Returns the result (2-D for the products and sums), or (result, S p) with p."""
    L = lib()
    L.eps_test_sparse_handle_op.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    g = _SparseHandleOp()
    g.op = op.encode("utf-8") if op is not None else None
    keep = []
    sm, sn = 0, 0
    if S is not None:
        payload = S if isinstance(S, (bytes, bytearray)) else S.proto.SerializeToString()
        buf = ctypes.create_string_buffer(bytes(payload), max(len(payload), 1))
        keep.append(buf)
        g.sparse_map, g.len = ctypes.cast(buf, ctypes.c_void_p), len(payload)
        if not isinstance(S, (bytes, bytearray)):
            blobs, nb = _blobs(S.data, keep)
            keep.append(blobs)
            g.data, g.ndata = ctypes.cast(blobs, ctypes.c_void_p), nb
            sm, sn = (S.n, S.m) if transpose else (S.m, S.n)
    g.transpose, g.scaled, g.scale = int(transpose), int(scale is not None), 1.0 if scale is None else scale
    if d is not None:
        d = np.asarray(d, dtype=np.float64)
        g.d_rows, g.d_cols = d.shape[0], (1 if d.ndim == 1 else d.shape[1])
        d = np.asfortranarray(d)
        keep.append(d)
        g.d = d.ctypes.data_as(ctypes.c_void_p)
    keep += _set_operands(g, (("p", p),))
    shape = {"apply": (sm, 1), "adjoint": (sn, 1), "sparse_dense": (sm, g.d_cols), "dense_sparse": (g.d_rows, sn)}.get(
        op, (sm, sn))
    out = np.full(max(shape[0] * shape[1], 1), np.nan)
    out2 = np.full(max(S.m, 1), np.nan) if p is not None and S is not None and not isinstance(S, (bytes, bytearray)) else None
    _check(L.eps_test_sparse_handle_op(ctypes.byref(g), out.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.c_int64(shape[0] * shape[1]),
                                       out2.ctypes.data_as(ctypes.c_void_p) if out2 is not None else None))
    del keep
    res = out[:shape[0] * shape[1]]
    res = res if op in ("apply", "adjoint") else res.reshape(shape, order="F")
    return res if p is None else (res, out2[:S.m])


def tv1d(v, lam):
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    x = np.empty_like(v)
    _check(lib().eps_tv1d(v.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(v.size),
                          ctypes.c_double(lam), x.ctypes.data_as(ctypes.c_void_p)))
    return x


def tv1d_batch(V, lam, axis=0):
    """The TV-1D prox of every column (axis=0) or every row (axis=1) of the 2-D array V, each on
    its own and all with the weight lam, in one device pass (eps_tv1d_batch).  Returns an array
    of V's shape."""
    V = np.asarray(V, dtype=np.float64)
    if V.ndim != 2:
        raise error("tv1d_batch: V must be a 2-D array, got %d dimension(s)" % V.ndim)
    if axis not in (0, 1):
        raise error("tv1d_batch: axis must be 0 or 1, got %r" % (axis,))
    # the slices one after the other: the columns of V (axis 0) or its rows (axis 1)
    S = np.ascontiguousarray(V.T if axis == 0 else V)
    count, length = S.shape
    X = np.empty_like(S)
    _check(lib().eps_tv1d_batch(S.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(length),
                                ctypes.c_size_t(count), ctypes.c_double(lam),
                                X.ctypes.data_as(ctypes.c_void_p)))
    return np.ascontiguousarray(X.T) if axis == 0 else X
