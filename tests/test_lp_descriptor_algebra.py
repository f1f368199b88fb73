"""The closed forms behind the two separable descriptors of the linear-program route (DESIGN.md 3.11 "A
linear term on x, a cone on z"; csrc/prox.h SeparableDesc::kLinear, kNonNegative) against the CPU
oracle's own AFFINE and NON_NEGATIVE operators, in numpy: with v the prox input on the term's
constraint row, a the constraint's scalar and alpha the term's weight,

  AFFINE(c^T x):                  x = (a v - alpha c) / a^2
  NON_NEGATIVE(h z + g):          z = (max(h v / a + g, 0) - g) / h

No GPU and no library: the oracle alone."""

import numpy as np
import pytest

from epsilon_amd import ir, wire
from epsilon_amd.wire import ProxFunction
from oracle import epsilon_oracle as orc

M, N = 7, 5


def solver_of(a_x, a_z, alpha, c, h, g):
    """affine(c^T x)[alpha] + non_negative(h z + g) + zero(C x' - z')  s.t.  x' + a_x x = 0, z' + a_z z = 0,
    initialised on the oracle: its operators are built, nothing is solved"""
    rng = np.random.RandomState(3)
    x, z = ir.variable(N, 1, "var:x"), ir.variable(M, 1, "var:z")
    xp, zp = ir.variable(N, 1, "separate:var:x:zero"), ir.variable(M, 1, "separate:var:z:zero")
    arg = ir.linear_map(ir.scalar(h, M), z)
    if g is not None:
        arg = ir.add(arg, ir.constant(g))
    terms = [ir.prox(ProxFunction.AFFINE, ir.linear_map(ir.dense_matrix(c.reshape(1, -1)), x), alpha=alpha),
             ir.prox(ProxFunction.NON_NEGATIVE, arg),
             ir.prox(ProxFunction.ZERO, ir.add(ir.linear_map(ir.dense_matrix(rng.randn(M, N)), xp),
                                               ir.linear_map(ir.scalar(-1, M), zp)))]
    cons = [ir.zero(ir.add(xp, ir.linear_map(ir.scalar(a_x, N), x))),
            ir.zero(ir.add(zp, ir.linear_map(ir.scalar(a_z, M), z)))]
    prob = ir.Problem(terms, cons)
    s = orc.create_solver(wire.Problem.FromString(prob.SerializeToString()), dict(prob.expression_data()),
                          wire.SolverParams())
    s.init()
    return s


@pytest.mark.parametrize("a", [-1.0, 1.0, -0.5, 2.5])
@pytest.mark.parametrize("alpha", [1.0, 0.3, 4.0])
def test_the_linear_term_is_its_closed_form(a, alpha):
    rng = np.random.RandomState(11)
    c = rng.randn(N)
    s = solver_of(a, -1.0, alpha, c, 1.0, None)
    u = orc.BlockVector()
    vx, vz = rng.randn(N), rng.randn(M)
    u.set(orc.constraint_key(0), vx)
    u.set(orc.constraint_key(1), vz)
    x = s.prox[0].apply(u)
    np.testing.assert_allclose(np.asarray(x("var:x")).ravel(), (a * vx - alpha * c) / a ** 2, rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("a", [-1.0, 1.0, -0.5, 2.5])
@pytest.mark.parametrize("h,offset", [(1.0, False), (1.0, True), (-2.0, True), (0.25, False)])
def test_the_cone_is_its_closed_form(a, h, offset):
    rng = np.random.RandomState(13)
    g = rng.randn(M) if offset else None
    s = solver_of(-1.0, a, 1.0, rng.randn(N), h, g)
    u = orc.BlockVector()
    vx, vz = rng.randn(N), rng.randn(M)
    u.set(orc.constraint_key(0), vx)
    u.set(orc.constraint_key(1), vz)
    z = np.asarray(s.prox[1].apply(u)("var:z")).ravel()
    g0 = g if offset else 0.0
    want = (np.maximum(h * vz / a + g0, 0.0) - g0) / h
    assert (h * z + g0 >= -1e-14).all() and (h * z + g0 > 1e-3).any() and (np.abs(h * z + g0) < 1e-14).any()
    np.testing.assert_allclose(z, want, rtol=1e-13, atol=1e-14)
