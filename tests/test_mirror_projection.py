"""CPU: tests/golden/projection_reference.py -- the dense mass, the composite-rule load and the dense solve the GPU tests of
mi_mass_apply / mi_mass_solve / mi_project_load / mi_state_project compare against -- anchored to what an L2 projection is:

  * its vectorised bases equal mirror.shape_at, its mass integrates 1 to the volume;
  * a polynomial of degree <= p is reproduced;
  * the free-dof residual (b - M w)_f is 0;
  * Pythagoras on the exact pairs: src_sq = dst_sq + int |w_src - w_dst|^2 (with all faces free and with dst's constraints a
    subset of what src's field satisfies);
  * projection equals interpolation when src's space lies in dst's.

It also records, for every mesh the GPU tests use, kappa_2(M_ff), kappa(D^-1 M_ff) and the iteration counts of the numpy
Jacobi-PCG at tol 1e-12 and 1e-14 (printed).  Recorded here: kappa_2 from 9 (one Q1 cell) to 935 (one perturbed Q4 cell: it grows
with the degree, not with the cell count), kappa(D^-1 M_ff) from 9 to 22.8 (largest for Q1, independent of h), 3 to 50 iterations.
Asserted is what the GPU tests lean on: kappa_2 < 1000, so that the solve bound kappa_2 (res + 64 eps) stays below 1e-9 at
tol 1e-12; kappa(D^-1 M_ff) <= 27 = 3^3, the bound of the diagonally scaled tensor-product Q1 mass on boxes, which the higher
degrees stay below; convergence well inside the default max_it of 500.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mirror as Mi  # noqa: E402
import point_eval_cases as PC  # noqa: E402
import projection_cases as PJ  # noqa: E402
import projection_reference as PR  # noqa: E402

FREE3, FREE2 = [0] * 6, [0] * 4


def _nodal(mesh, f):
    return f(mesh.coords).reshape(-1)


@pytest.mark.parametrize("dim,p", [(2, 1), (2, 4), (3, 2), (3, 3)])
def test_bases_equal_shape_at(dim, p):
    rng = np.random.default_rng(dim * 10 + p)
    xi = rng.uniform(-0.1, 1.1, (7, dim))
    N = PR.shape_many(dim, p, xi)
    for k in range(len(xi)):
        ref, _ = Mi.shape_at(dim, p, Mi.feq_nodes(p), xi[k])
        assert np.abs(N[k] - ref).max() < 1e-13


@pytest.mark.parametrize("dim,p,perturbed", [(2, 2, True), (3, 1, True), (3, 3, False)])
def test_mass_integrates_one_to_the_volume(dim, p, perturbed):
    c = PC.make_mesh(dim, p, PJ.REPS[dim], perturbed)
    M = PR.scalar_mass(c["mesh"])
    vol = np.prod(np.array(c["hi"]) - np.array(c["lo"]))
    assert np.abs(M - M.T).max() == 0.0 or np.abs(M - M.T).max() < 1e-18
    if not perturbed:  # (a perturbed mesh moves its boundary vertices too)
        assert abs(M.sum() - vol) < 1e-14 * vol * M.shape[0]
    xi, w, _, _ = Mi._rule(dim, p, p + 2)
    assert abs(M.sum() - PR.cell_jxw(c["mesh"], xi, w).sum()) < 1e-13 * vol


@pytest.mark.parametrize("dim,p,perturbed,sub", [(2, 3, False, 1), (3, 2, False, 2), (3, 1, False, 3), (2, 2, True, 1)])
def test_polynomial_is_reproduced(dim, p, perturbed, sub):
    """src: the same box with sub x the cells (boxes) or the same lattice (perturbed), all faces free; a polynomial of degree <= p
    lies in both spaces on boxes; on the perturbed lattice the affine field does"""
    roles = FREE3[:2 * dim]
    cd = PC.make_mesh(dim, p, PJ.REPS[dim], perturbed, roles=roles)
    cs = PC.make_mesh(dim, p, PJ.REPS[dim], perturbed, roles=roles, refine=1 if perturbed else sub)
    rng = np.random.default_rng(5)
    f = PC.Affine(dim, rng) if perturbed else PC.Poly(dim, p, cd["hi"], rng)
    md, ms = cd["mesh"], cs["mesh"]
    b, src_sq = PR.load(md, ms, _nodal(ms, f), sub)
    w = PR.solve(PR.scalar_mass(md), b, dim, md.constrained)
    ref = _nodal(md, f)
    assert np.abs(w - ref).max() < 1e-11 * np.abs(ref).max()
    assert PR.error_sq(md, ms, _nodal(ms, f), w, sub) < 1e-22 * src_sq


@pytest.mark.parametrize("case", PJ.EXACT_PAIRS, ids=PJ.pair_id)
def test_orthogonality_and_pythagoras(case):
    cs, cd, sub = PJ.pair(case)
    ms, md = cs["mesh"], cd["mesh"]
    w_src = PJ.source_state(cs)[:2]
    b, src_sq = PR.load(md, ms, w_src, sub)
    M = PR.scalar_mass(md)
    w = PR.solve(M, b, md.dim, md.constrained)
    r = (b - PR.mass_apply(M, w, md.dim))[:, ~md.constrained]
    assert np.abs(r).max() < 1e-13 * np.abs(b).max()
    dst_sq = np.einsum("kn,kn->k", w, PR.mass_apply(M, w, md.dim))
    err = PR.error_sq(md, ms, w_src, w, sub)
    print("src_sq", src_sq, "dst_sq", dst_sq, "err", err)
    assert np.all(dst_sq <= src_sq * (1 + 1e-12))
    assert np.abs(src_sq - dst_sq - err).max() < 1e-12 * src_sq.max()


def test_projection_equals_interpolation_when_nested():
    """3 x 2 x 3 -> 6 x 4 x 6 Q2 on boxes: src's space lies in dst's, the projection is src's field itself"""
    cs, cd = PC.make_mesh(3, 2, PJ.REPS[3], False), PC.make_mesh(3, 2, PJ.REPS[3], False, refine=2)
    ms, md = cs["mesh"], cd["mesh"]
    w_src = PJ.source_state(cs)[0]
    b, _ = PR.load(md, ms, w_src, 1)
    w = PR.solve(PR.scalar_mass(md), b, 3, md.constrained)
    conn = np.array([c[0] for c in md.cells])
    interp = np.zeros(md.n)
    nodes1 = Mi.feq_nodes(2)
    corners = np.array([[nodes1[(a // 3 ** d) % 3] for d in range(3)] for a in range(27)])
    val = PR.source_values(md, ms, w_src, corners)  # [E, 27, 3]: src at dst's support points
    for c in range(3):
        interp[conn * 3 + c] = val[:, :, c]
    interp[md.constrained] = 0.0
    assert np.abs(w - interp).max() < 1e-11 * np.abs(interp).max()


@pytest.mark.parametrize("key", PJ.MASS_MESHES, ids=PJ.mesh_id)
def test_conditioning_and_pcg_iterations(key):
    c = PJ.mass_mesh(key)
    m = c["mesh"]
    M = PR.scalar_mass(m)
    worst = dict(k2=0.0, kd=0.0, it12=0, it14=0)
    rng = np.random.default_rng(3)
    for A in PR.free_blocks(M, m.dim, m.constrained):
        ev = np.linalg.eigvalsh(A)
        d = 1.0 / np.sqrt(np.diag(A))
        evd = np.linalg.eigvalsh(A * d[:, None] * d[None, :])
        b = rng.standard_normal(A.shape[0])
        x12, it12 = PR.jacobi_pcg(A, b, 1e-12, 500)
        x14, it14 = PR.jacobi_pcg(A, b, 1e-14, 500)
        assert np.linalg.norm(b - A @ x14) <= 3e-14 * np.linalg.norm(b)
        worst = dict(k2=max(worst["k2"], ev[-1] / ev[0]), kd=max(worst["kd"], evd[-1] / evd[0]), it12=max(worst["it12"], it12),
                     it14=max(worst["it14"], it14))
    print("%s: kappa_2(M_ff) %.1f  kappa(D^-1 M_ff) %.2f  PCG iterations %d (1e-12) %d (1e-14)" %
          (PJ.mesh_id(key), worst["k2"], worst["kd"], worst["it12"], worst["it14"]))
    assert worst["k2"] < 1000.0
    assert worst["kd"] <= 27.0
    assert worst["it14"] <= 60
