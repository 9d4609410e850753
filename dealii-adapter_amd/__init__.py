"""ctypes plumbing over libmi_elasticity.so (C-ABI: include/mi_elasticity.h).

This module is test/bench plumbing only: the product's host side is C++ (dealii-adapter_amd/host/), as in
the reference.  There is no CPU fallback: if the HIP library is missing or no device is visible, loading or
context creation raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("MI_LIB") or os.path.join(PKG_DIR, "libmi_elasticity.so")  # MI_LIB: A/B of two builds in one job (tools)
HEADER = os.path.join(ROOT, "include", "mi_elasticity.h")

MI_OK, MI_EINVAL, MI_EHIP, MI_ENOCONV_LIN, MI_ENOCONV_NR, MI_ECOMM = 0, -1, -2, -3, -4, -5
FACE_FREE, FACE_CLAMPED, FACE_INTERFACE, FACE_ZCLAMP = 0, 1, 7, 8
STRESS_NEOHOOKE, STRESS_LINEAR = 0, 1  # mi_stress_field's models
STRESS_AT_RAW, STRESS_AT_RECOVERED = 0, 1  # mi_evaluate_stress's kinds
(V_U, V_U_OLD, V_V, V_V_OLD, V_A, V_A_OLD, V_STRESS, V_DELTA, V_NEWTON, V_RHS) = range(10)
(T_ASSEMBLE_CELLS, T_ASSEMBLE_TOTAL, T_SPMV, T_CG_VECTOR, T_CG_TOTAL, T_NEWMARK, T_STEP, T_ASSEMBLE_DIAG, T_ASSEMBLE_RESIDUAL,
 T_SPMV_PRECOND, T_EBE_LAUNCH, T_COUNT) = range(12)
TIMING_NAMES = ["assemble_cells", "assemble_total", "spmv", "cg_vector", "cg_total", "newmark", "step", "assemble_diag",
                "assemble_residual", "spmv_precond", "ebe_launch"]


class MeshDesc(C.Structure):
    _fields_ = [("dim", C.c_int32), ("degree", C.c_int32), ("reps", C.c_int32 * 3), ("lo", C.c_double * 3),
                ("hi", C.c_double * 3), ("face_role", C.c_int32 * 6), ("vertex_perturbation", C.POINTER(C.c_double))]


class MaterialDesc(C.Structure):
    _fields_ = [("mu", C.c_double), ("nu", C.c_double), ("rho", C.c_double), ("body_force", C.c_double * 3)]


class NewmarkDesc(C.Structure):
    _fields_ = [("beta", C.c_double), ("gamma", C.c_double), ("delta_t", C.c_double)]


class CommDesc(C.Structure):
    _fields_ = [("rank", C.c_int32), ("size", C.c_int32), ("nccl_unique_id", C.c_void_p), ("cut_axis", C.c_int32)]


class PartitionInfo(C.Structure):
    _fields_ = [("z0", C.c_int32), ("z1", C.c_int32), ("local_layers", C.c_int32), ("plane_nodes", C.c_int64),
                ("node_offset", C.c_int64), ("nnodes_global", C.c_int64), ("nnodes_local", C.c_int64),
                ("own_begin", C.c_int64), ("own_end", C.c_int64), ("up_send", C.c_int64), ("up_send_n", C.c_int64),
                ("up_recv", C.c_int64), ("up_recv_n", C.c_int64), ("down_send", C.c_int64), ("down_send_n", C.c_int64),
                ("down_recv", C.c_int64), ("down_recv_n", C.c_int64), ("local_reps", C.c_int32 * 3),
                ("local_lo", C.c_double * 3), ("local_hi", C.c_double * 3), ("local_face_role", C.c_int32 * 6)]


class SolverDesc(C.Structure):
    _fields_ = [("tol_lin", C.c_double), ("max_iterations_lin", C.c_double), ("max_iterations_NR", C.c_int32),
                ("tol_f", C.c_double), ("tol_u", C.c_double)]


class StepInfo(C.Structure):
    _fields_ = [("newton_iterations", C.c_int32), ("assemblies", C.c_int32), ("lin_its_total", C.c_int32),
                ("converged", C.c_int32), ("res_norm", C.c_double), ("res_abs", C.c_double),
                ("upd_norm", C.c_double), ("upd_abs", C.c_double), ("lin_its", C.c_int32 * 16),
                ("lin_res", C.c_double * 16)]


class Timings(C.Structure):
    _fields_ = [("ms", C.c_double * T_COUNT), ("count", C.c_int64 * T_COUNT)]


class MgLevelDesc(C.Structure):
    _fields_ = [("degree", C.c_int32), ("reps", C.c_int32 * 3), ("n_dofs", C.c_int64), ("lmax", C.c_double),
                ("interval_ratio", C.c_double), ("smoother_degree", C.c_int32), ("exact_solve", C.c_int32),
                ("distributed", C.c_int32), ("reserved", C.c_int32)]


class EnergyInfo(C.Structure):
    _fields_ = [("strain", C.c_double), ("kinetic", C.c_double), ("body", C.c_double), ("reserved", C.c_double)]


class StressErrorInfo(C.Structure):
    _fields_ = [("error", C.c_double), ("norm", C.c_double), ("relative", C.c_double), ("max_cell_error", C.c_double),
                ("max_cell", C.c_int64), ("reserved", C.c_int64)]


class ReactionInfo(C.Structure):
    _VECTORS = ("about", "reaction", "reaction_moment", "unbalanced", "unbalanced_moment", "inertia", "inertia_moment", "body",
                "body_moment", "load", "load_moment")
    _fields_ = ([(k, C.c_double * 3) for k in _VECTORS] +
                [("internal_abs", C.c_double), ("max_unbalanced", C.c_double), ("max_reaction", C.c_double),
                 ("max_reaction_node", C.c_int64)])


class ProjectInfo(C.Structure):
    _fields_ = [("its", C.c_int32), ("sub", C.c_int32), ("n_points", C.c_int64), ("res", C.c_double),
                ("src_sq", C.c_double * 6), ("dst_sq", C.c_double * 6)]


class ExplicitInfo(C.Structure):
    _fields_ = [("steps_done", C.c_int32), ("inverted_step", C.c_int32), ("dt", C.c_double), ("kinetic_lumped", C.c_double)]


class MiError(RuntimeError):
    def __init__(self, code, msg, partial=None):
        super().__init__("mi_elasticity error %d: %s" % (code, msg))
        self.code = code
        self.partial = partial  # what the call wrote before it gave up (Context.linear_modes on MI_ENOCONV_LIN), else None


def build(force=False):
    """compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)"""
    if force:
        subprocess.check_call(["make", "-C", PKG_DIR, "clean"])
    subprocess.check_call(["make", "-C", PKG_DIR, "-j4", "all"])


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `make -C dealii-adapter_amd` (no CPU fallback exists)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        dp, i32p, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
        L.mi_ctx_create.restype = C.c_int
        L.mi_ctx_create.argtypes = [C.POINTER(MeshDesc), C.POINTER(MaterialDesc), C.POINTER(NewmarkDesc), C.c_int,
                                    C.POINTER(CommDesc), C.POINTER(vp)]
        L.mi_ctx_destroy.restype = None
        L.mi_ctx_destroy.argtypes = [vp]
        L.mi_last_error.restype = C.c_char_p
        L.mi_last_error.argtypes = [vp]
        for f in ("mi_n_dofs", "mi_n_nodes", "mi_n_cells", "mi_nnz"):
            getattr(L, f).restype = C.c_int64
            getattr(L, f).argtypes = [vp]
        for f in ("mi_n_colours", "mi_n_interface_nodes", "mi_newton_begin_step", "mi_update_acceleration",
                  "mi_newmark_finish_step", "mi_state_save", "mi_state_restore", "mi_reset_timings"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [vp]
        L.mi_get_node_coords.argtypes = [vp, dp]
        L.mi_get_constrained.argtypes = [vp, C.POINTER(C.c_uint8)]
        L.mi_get_interface_nodes.argtypes = [vp, i32p, dp]
        L.mi_set_interface_traction.argtypes = [vp, C.c_int, dp]
        L.mi_get_interface_displacement.argtypes = [vp, C.c_int, dp]
        L.mi_assemble.argtypes = [vp, dp]
        L.mi_assemble_residual.argtypes = [vp, dp]
        L.mi_assemble_residual.restype = C.c_int
        L.mi_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi_comm_info.restype = C.c_int
        L.mi_comm_broadcast.argtypes = [vp, C.POINTER(C.c_double), C.c_int32]
        L.mi_comm_broadcast.restype = C.c_int
        L.mi_cg_solve.argtypes = [vp, C.c_double, C.c_int64, C.POINTER(C.c_int), dp]
        L.mi_apply_newton_update.argtypes = [vp, dp]
        L.mi_direct_solve.argtypes = [vp, dp]
        L.mi_direct_solve.restype = C.c_int
        L.mi_newmark_step.argtypes = [vp, C.POINTER(SolverDesc), C.POINTER(StepInfo)]
        L.mi_vec_get.argtypes = [vp, C.c_int, dp, C.c_int64]
        L.mi_vec_set.argtypes = [vp, C.c_int, dp, C.c_int64]
        L.mi_matrix_get_csr.argtypes = [vp, C.POINTER(C.c_int64), i32p, dp]
        L.mi_spmv.argtypes = [vp, dp, dp]
        L.mi_spmm.argtypes = [vp, C.c_int, dp, dp]
        L.mi_spmm.restype = C.c_int
        L.mi_bench_spmm.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, dp]
        L.mi_bench_spmm.restype = C.c_int
        L.mi_get_diagonal_blocks.argtypes = [vp, dp]
        L.mi_get_diagonal_blocks.restype = C.c_int
        L.mi_linear_setup.argtypes = [vp, C.c_double]
        L.mi_linear_step.argtypes = [vp, C.c_int, C.c_double, C.c_int64, C.POINTER(C.c_int), dp]
        L.mi_linear_matrix_get_csr.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), i32p, dp]
        L.mi_linear_apply.argtypes = [vp, C.c_int, dp, dp]
        L.mi_linear_get_diagonal.argtypes = [vp, dp]
        for f in ("mi_linear_setup", "mi_linear_step", "mi_linear_matrix_get_csr", "mi_linear_apply", "mi_linear_get_diagonal"):
            getattr(L, f).restype = C.c_int
        L.mi_linear_get_diagonal_blocks.argtypes = [vp, dp]
        L.mi_linear_mg_n_levels.argtypes = [vp]
        L.mi_linear_mg_level_describe.argtypes = [vp, C.c_int, C.POINTER(MgLevelDesc)]
        L.mi_linear_mg_level_context.argtypes = [vp, C.c_int, C.POINTER(vp)]
        for f in ("mi_linear_get_diagonal_blocks", "mi_linear_mg_n_levels", "mi_linear_mg_level_describe",
                  "mi_linear_mg_level_context"):
            getattr(L, f).restype = C.c_int
        for f in ("mi_energy", "mi_linear_energy"):
            getattr(L, f).argtypes = [vp, C.POINTER(EnergyInfo)]
            getattr(L, f).restype = C.c_int
        L.mi_stress_field.argtypes = [vp, C.c_int, dp, dp, dp]
        L.mi_stress_field.restype = C.c_int
        L.mi_stress_error.argtypes = [vp, C.c_int, C.POINTER(StressErrorInfo), dp, dp]
        L.mi_stress_error.restype = C.c_int
        L.mi_reactions.argtypes = [vp, C.c_int, dp, C.POINTER(ReactionInfo), dp, dp]
        L.mi_reactions.restype = C.c_int
        L.mi_evaluate_points.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.c_int64, dp, dp, dp, C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64)]
        L.mi_evaluate_points.restype = C.c_int
        L.mi_evaluate_stress.argtypes = [vp, C.c_int, C.c_int, C.c_int64, dp, dp, dp, dp, dp, C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64)]
        L.mi_evaluate_stress.restype = C.c_int
        L.mi_principal_stress.argtypes = [vp, C.c_int64, dp, dp, dp]
        L.mi_principal_stress.restype = C.c_int
        L.mi_state_transfer.argtypes = [vp, vp]
        L.mi_state_transfer.restype = C.c_int
        L.mi_mass_apply.argtypes = [vp, C.c_int, C.c_int, dp, dp]
        L.mi_mass_solve.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_double, C.c_int, C.POINTER(C.c_int), dp]
        L.mi_project_load.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int), C.c_int, dp]
        L.mi_state_project.argtypes = [vp, vp, C.c_int, C.c_double, C.c_int, C.POINTER(ProjectInfo)]
        for f in ("mi_mass_apply", "mi_mass_solve", "mi_project_load", "mi_state_project"):
            getattr(L, f).restype = C.c_int
        L.mi_linear_modes.argtypes = [vp, C.c_int, C.c_double, C.c_int, dp, dp, dp, C.POINTER(C.c_int)]
        L.mi_block_gram.argtypes = [vp, C.c_int64, dp, C.c_int, dp, C.c_int, dp]
        L.mi_block_combine.argtypes = [vp, C.c_int64, dp, C.c_int, dp, C.c_int, dp]
        L.mi_dense_sym_eig.argtypes = [C.c_int, dp, dp, dp, dp]
        L.mi_tangent_modes.argtypes = [vp, C.c_int, C.c_double, C.c_int, dp, dp, dp, C.POINTER(C.c_int)]
        for f in ("mi_linear_modes", "mi_tangent_modes", "mi_block_gram", "mi_block_combine", "mi_dense_sym_eig"):
            getattr(L, f).restype = C.c_int
        L.mi_explicit_setup.argtypes = [vp, C.c_double, C.c_int]
        L.mi_explicit_run.argtypes = [vp, C.c_int, C.POINTER(ExplicitInfo)]
        L.mi_explicit_get_mass.argtypes = [vp, dp]
        L.mi_explicit_stable_dt.argtypes = [vp, C.c_int, dp, dp]
        for f in ("mi_explicit_setup", "mi_explicit_run", "mi_explicit_get_mass", "mi_explicit_stable_dt"):
            getattr(L, f).restype = C.c_int
        L.mi_set_profiling.argtypes = [vp, C.c_int]
        L.mi_get_timings.argtypes = [vp, C.POINTER(Timings)]
        L.mi_partition_describe.restype = C.c_int
        L.mi_partition_describe.argtypes = [C.POINTER(MeshDesc), C.c_int, C.c_int, C.POINTER(PartitionInfo)]
        L.mi_partition_spmv_rows.restype = C.c_int
        L.mi_partition_spmv_rows.argtypes = [C.POINTER(MeshDesc), C.c_int, C.c_int, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int64]
        L.mi_comm_unique_id.restype = C.c_int
        L.mi_comm_unique_id.argtypes = [C.c_void_p]
        L.mi_set_tuning.argtypes = [vp, C.c_char_p, C.c_int]
        L.mi_set_tuning.restype = C.c_int
        L.mi_get_tuning.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
        L.mi_get_tuning.restype = C.c_int
        L.mi_bench_spmv.argtypes = [vp, C.c_int, dp]
        L.mi_bench_assemble.argtypes = [vp, C.c_int, dp]
        L.mi_mg_n_levels.argtypes = [vp]
        L.mi_mg_level_describe.argtypes = [vp, C.c_int, C.POINTER(MgLevelDesc)]
        L.mi_mg_level_context.argtypes = [vp, C.c_int, C.POINTER(vp)]
        for f in ("mi_mg_n_levels", "mi_mg_level_describe", "mi_mg_level_context"):
            getattr(L, f).restype = C.c_int
        for f in ("mi_get_node_coords", "mi_get_constrained", "mi_get_interface_nodes", "mi_set_interface_traction",
                  "mi_get_interface_displacement", "mi_assemble", "mi_cg_solve", "mi_apply_newton_update",
                  "mi_newmark_step", "mi_vec_get", "mi_vec_set", "mi_matrix_get_csr", "mi_spmv", "mi_set_profiling",
                  "mi_get_timings", "mi_bench_spmv", "mi_bench_assemble"):
            getattr(L, f).restype = C.c_int
        _lib = L
    return _lib


def declared_symbols():
    """entry points declared in include/mi_elasticity.h"""
    import re
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", txt)))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def mesh_desc(dim, degree, reps, lo, hi, face_role):
    md = MeshDesc()
    md.dim, md.degree = dim, degree
    reps = tuple(reps) + (1,) * (3 - len(reps))
    lo = tuple(lo) + (0.0,) * (3 - len(lo))
    hi = tuple(hi) + (0.0,) * (3 - len(hi))
    for i in range(3):
        md.reps[i], md.lo[i], md.hi[i] = reps[i], lo[i], hi[i]
    for i in range(6):
        md.face_role[i] = face_role[i]
    return md


def partition_describe(md, rank, size):
    """host-only slab description (works without a GPU)"""
    info = PartitionInfo()
    rc = lib().mi_partition_describe(C.byref(md), rank, size, C.byref(info))
    if rc != MI_OK:
        raise MiError(rc, lib().mi_last_error(None).decode())
    return info


def partition_spmv_rows(md, rank, size):
    """host-only: (rows, n_interior_slots) -- SpMV row order of a slab, interior rows first (-1 = padding)"""
    ns, ni = C.c_int64(), C.c_int64()
    rc = lib().mi_partition_spmv_rows(C.byref(md), rank, size, C.byref(ns), C.byref(ni), None, 0)
    if rc != MI_OK:
        raise MiError(rc, lib().mi_last_error(None).decode())
    rows = np.zeros(ns.value * 64, dtype=np.int32)
    rc = lib().mi_partition_spmv_rows(C.byref(md), rank, size, C.byref(ns), C.byref(ni),
                                      rows.ctypes.data_as(C.POINTER(C.c_int32)), rows.size)
    if rc != MI_OK:
        raise MiError(rc, lib().mi_last_error(None).decode())
    return rows, ni.value * 64


def comm_unique_id():
    buf = C.create_string_buffer(128)
    rc = lib().mi_comm_unique_id(buf)
    if rc != MI_OK:
        raise MiError(rc, lib().mi_last_error(None).decode())
    return buf.raw


def block_gram(ctx, a, b):
    """a^T b of two tall blocks [n, ma], [n, mb] through the device's block_gram (ma, mb <= 60)"""
    a, b = np.asfortranarray(a, dtype=np.float64), np.asfortranarray(b, dtype=np.float64)
    c = np.zeros((a.shape[1], b.shape[1]))
    ctx._chk(lib().mi_block_gram(ctx.h, a.shape[0], _dp(a), a.shape[1], _dp(b), b.shape[1], _dp(c)))
    return c


def block_combine(ctx, s, coef):
    """s coef of a tall block [n, ks] and coefficients [ks, my] through the device's block_combine (ks <= 60, my <= 20)"""
    s, coef = np.asfortranarray(s, dtype=np.float64), np.ascontiguousarray(coef, dtype=np.float64)
    y = np.zeros((s.shape[0], coef.shape[1]), order="F")
    ctx._chk(lib().mi_block_combine(ctx.h, s.shape[0], _dp(s), s.shape[1], _dp(coef), coef.shape[1], _dp(y)))
    return y


def dense_sym_eig(A, B):
    """(w, V) with A V = B V diag(w), V^T B V = I, w ascending: the host's Cholesky + cyclic Jacobi (n <= 64; no device)"""
    A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    n = A.shape[0]
    w, V = np.zeros(n), np.zeros((n, n))
    rc = lib().mi_dense_sym_eig(n, _dp(A), _dp(B), _dp(w), _dp(V))
    if rc != MI_OK:
        raise MiError(rc, lib().mi_last_error(None).decode())
    return w, V.T.copy()  # (eigenvector j is row j of the C array)


class LevelView:
    """a level of the multigrid hierarchy, borrowed from its context (mi_mg_level_context): read methods only.  It dies with
    the next rebuild of the hierarchy and with the context; close() does nothing."""

    def __init__(self, owner, handle):
        self._owner = owner  # keeps the context alive
        self.h = handle
        L = lib()
        self.dim = owner.dim
        self.n = L.mi_n_dofs(self.h)
        self.nnodes = L.mi_n_nodes(self.h)
        self.nnz = L.mi_nnz(self.h)

    def close(self):
        pass

    def _chk(self, rc):
        if rc != MI_OK:
            raise MiError(rc, lib().mi_last_error(self.h).decode())

    @property
    def constrained(self):
        return Context.constrained.fget(self)

    def total_displacement(self):
        """levels >= 1: the state the level's operator was assembled at (u + du interpolated down).  Level 0 is the fine
        context itself and this is its V_U alone; its tangent was assembled at V_U + V_DELTA"""
        return Context.get(self, V_U)

    def csr(self):
        return Context.csr(self)

    def diagonal_blocks(self):
        return Context.diagonal_blocks(self)

    def get_tuning(self, key):
        """read-backs of the level's own context ("spmv_lds_launches", "spmv_split_launches": the kernel its products run)"""
        return Context.get_tuning(self, key)

    # a level of the linear model's hierarchy (mi_linear_mg_level_context)
    def linear_csr(self, which):
        return Context.linear_csr(self, which)

    def linear_diagonal_blocks(self):
        return Context.linear_diagonal_blocks(self)


class Context:
    """one device context = one (sub)domain of the structural problem on one GPU"""

    def __init__(self, dim=3, degree=2, reps=(4, 4, 4), lo=(0, 0, 0), hi=(1, 1, 1), face_role=None, mu=0.5e6, nu=0.4,
                 rho=1000.0, body_force=(0, 0, 0), beta=0.25, gamma=0.5, delta_t=0.005, device=0, perturb=None,
                 slabs=1, rank=None, world=1, unique_id=None, cut_axis=0):
        """slabs > 1: that many slabs inside this process (test mode); rank/world/unique_id: one slab per process
        over RCCL; cut_axis: 0 automatic (direction with most cell layers, ties: the last), 1 / 2 / 3 = x / y / z"""
        L = lib()
        md, mat, nm = MeshDesc(), MaterialDesc(), NewmarkDesc()
        md.dim, md.degree = dim, degree
        reps = tuple(reps) + (1,) * (3 - len(reps))
        lo = tuple(lo) + (0.0,) * (3 - len(lo))
        hi = tuple(hi) + (0.0,) * (3 - len(hi))
        if face_role is None:
            face_role = [FACE_CLAMPED] + [FACE_INTERFACE] * 5
        for i in range(3):
            md.reps[i], md.lo[i], md.hi[i], mat.body_force[i] = reps[i], lo[i], hi[i], body_force[i]
        for i in range(6):
            md.face_role[i] = face_role[i]
        self._perturb = None
        if perturb is not None:
            self._perturb = np.ascontiguousarray(perturb, dtype=np.float64)
            md.vertex_perturbation = _dp(self._perturb)
        mat.mu, mat.nu, mat.rho = mu, nu, rho
        nm.beta, nm.gamma, nm.delta_t = beta, gamma, delta_t
        self.h = C.c_void_p()
        comm = None
        if slabs > 1:
            comm = CommDesc(-1, slabs, None, cut_axis)
        elif world > 1 or unique_id is not None:
            self._uid = C.create_string_buffer(unique_id, 128)
            comm = CommDesc(rank or 0, world, C.cast(self._uid, C.c_void_p), cut_axis)
        rc = L.mi_ctx_create(C.byref(md), C.byref(mat), C.byref(nm), device, C.byref(comm) if comm else None,
                             C.byref(self.h))
        if rc != MI_OK:
            self.h = None
            raise MiError(rc, L.mi_last_error(None).decode())
        self.dim = dim
        self.n = L.mi_n_dofs(self.h)
        self.nnodes = L.mi_n_nodes(self.h)
        self.ncells = L.mi_n_cells(self.h)
        self.nnz = L.mi_nnz(self.h)

    def close(self):
        if getattr(self, "h", None):
            lib().mi_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc != MI_OK:
            raise MiError(rc, lib().mi_last_error(self.h).decode())

    @property
    def coords(self):
        x = np.zeros((self.nnodes, self.dim))
        self._chk(lib().mi_get_node_coords(self.h, _dp(x)))
        return x

    @property
    def constrained(self):
        f = np.zeros(self.n, dtype=np.uint8)
        self._chk(lib().mi_get_constrained(self.h, f.ctypes.data_as(C.POINTER(C.c_uint8))))
        return f.astype(bool)

    def interface(self):
        k = lib().mi_n_interface_nodes(self.h)
        ids = np.zeros(k, dtype=np.int32)
        xyz = np.zeros((k, self.dim))
        self._chk(lib().mi_get_interface_nodes(self.h, ids.ctypes.data_as(C.POINTER(C.c_int32)), _dp(xyz)))
        return ids, xyz

    def set_interface_traction(self, t):
        k = lib().mi_n_interface_nodes(self.h)
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (k, self.dim)))
        self._chk(lib().mi_set_interface_traction(self.h, k, _dp(t)))

    def get_interface_displacement(self):
        k = lib().mi_n_interface_nodes(self.h)
        out = np.zeros((k, self.dim))
        self._chk(lib().mi_get_interface_displacement(self.h, k, _dp(out)))
        return out

    def get(self, which):
        v = np.zeros(self.n)
        self._chk(lib().mi_vec_get(self.h, which, _dp(v), self.n))
        return v

    def set(self, which, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        self._chk(lib().mi_vec_set(self.h, which, _dp(v), self.n))

    def newton_begin_step(self):
        self._chk(lib().mi_newton_begin_step(self.h))

    def update_acceleration(self):
        self._chk(lib().mi_update_acceleration(self.h))

    def assemble(self):
        r = C.c_double(0)
        self._chk(lib().mi_assemble(self.h, C.byref(r)))
        return r.value

    def assemble_residual(self):
        r = C.c_double(0)
        self._chk(lib().mi_assemble_residual(self.h, C.byref(r)))
        return r.value

    def comm_info(self):
        """(slabs of the decomposition, ncclCommCount of the RCCL communicator or 0)"""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(lib().mi_comm_info(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def cg_solve(self, rel_tol=1e-6, max_it=None):
        its, res = C.c_int(0), C.c_double(0)
        rc = lib().mi_cg_solve(self.h, rel_tol, self.n if max_it is None else max_it, C.byref(its), C.byref(res))
        if rc not in (MI_OK, MI_ENOCONV_LIN):
            self._chk(rc)
        return rc, its.value, res.value

    def direct_solve(self):
        """banded Cholesky of the current tangent + substitution (mi_direct_solve); returns the status code"""
        r = C.c_double(0)
        rc = lib().mi_direct_solve(self.h, C.byref(r))
        if rc not in (MI_OK, MI_EINVAL, MI_ENOCONV_LIN):
            self._chk(rc)
        return rc

    def apply_newton_update(self):
        r = C.c_double(0)
        self._chk(lib().mi_apply_newton_update(self.h, C.byref(r)))
        return r.value

    def newmark_finish_step(self):
        self._chk(lib().mi_newmark_finish_step(self.h))

    def newmark_step(self, tol_lin=1e-6, max_it_mult=1.0, max_it_nr=10, tol_f=1e-9, tol_u=1e-6, check=True):
        s, info = SolverDesc(), StepInfo()
        s.tol_lin, s.max_iterations_lin, s.max_iterations_NR, s.tol_f, s.tol_u = (tol_lin, max_it_mult, max_it_nr,
                                                                                  tol_f, tol_u)
        rc = lib().mi_newmark_step(self.h, C.byref(s), C.byref(info))
        if check:
            self._chk(rc)
        return rc, info

    def comm_broadcast(self, values):
        """values of rank 0 to every rank (collective; returns the received array)"""
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._chk(lib().mi_comm_broadcast(self.h, _dp(v), v.size))
        return v

    def energy(self):
        """strain energy, kinetic energy and body-force potential of the committed state (V_U, V_V) of the nonlinear model"""
        e = EnergyInfo()
        self._chk(lib().mi_energy(self.h, C.byref(e)))
        return dict(strain=e.strain, kinetic=e.kinetic, body=e.body)

    def stress_field(self, model=STRESS_NEOHOOKE):
        """(sigma[n_nodes, ncomp], von_mises[n_nodes], weight[n_nodes]) of the committed state V_U: the lumped L2 projection of
        the Cauchy stress (STRESS_NEOHOOKE) or of lambda tr(eps) I + 2 mu eps (STRESS_LINEAR) onto the nodes; components
        xx, yy, zz, xy, xz, yz in 3D, xx, yy, xy in 2D"""
        ncomp = self.dim * (self.dim + 1) // 2
        sigma, vm, w = np.zeros((self.nnodes, ncomp)), np.zeros(self.nnodes), np.zeros(self.nnodes)
        self._chk(lib().mi_stress_field(self.h, model, _dp(sigma), _dp(vm), _dp(w)))
        return sigma, vm, w

    def stress_error(self, model=STRESS_NEOHOOKE, cells=True):
        """the Zienkiewicz-Zhu error indicator of stress_field(model): dict(error, norm, relative, max_cell_error, max_cell,
        eta_cell, norm_cell) -- eta, n, eta / sqrt(n^2 + eta^2), the largest eta_K and its lexicographic cell id, and with
        cells=True eta_K and n_K of every cell in lexicographic order (x fastest), else None.  An indicator, not a bound"""
        info = StressErrorInfo()
        eta, nrm = (np.zeros(self.ncells), np.zeros(self.ncells)) if cells else (None, None)
        self._chk(lib().mi_stress_error(self.h, model, C.byref(info), _dp(eta) if cells else None, _dp(nrm) if cells else None))
        return dict(error=info.error, norm=info.norm, relative=info.relative, max_cell_error=info.max_cell_error,
                    max_cell=int(info.max_cell), eta_cell=eta, norm_cell=nrm)

    def reactions(self, model=STRESS_NEOHOOKE, about=None, forces=True, terms=False):
        """support reactions and load resultants of the committed state (mi_reactions): a dict of the struct's fields -- about,
        reaction, unbalanced, inertia, body, load and their *_moment as arrays of 3; internal_abs, max_unbalanced, max_reaction,
        max_reaction_node -- plus forces [n] = internal + inertia - body - load on every dof and terms [4, n] = internal,
        inertia, body, load (None unless asked).  about: the point the moments are taken about (default: the origin)"""
        info = ReactionInfo()
        x0 = None if about is None else np.ascontiguousarray(about, dtype=np.float64).reshape(self.dim)
        f = np.zeros(self.n) if forces else None
        t = np.zeros((4, self.n)) if terms else None
        self._chk(lib().mi_reactions(self.h, model, None if x0 is None else _dp(x0), C.byref(info), _dp(f) if forces else None,
                                     _dp(t) if terms else None))
        out = {k: np.array(getattr(info, k)) for k in ReactionInfo._VECTORS}
        out.update(internal_abs=info.internal_abs, max_unbalanced=info.max_unbalanced, max_reaction=info.max_reaction,
                   max_reaction_node=int(info.max_reaction_node), forces=f, terms=t)
        return out

    def evaluate(self, which, points, gradients=False):
        """(values, gradients, cell, n_outside) of the state vectors `which` (one V_* / L_* id or a sequence) at the points
        [npts, dim] of the reference configuration: values [n_which, npts, dim], gradients [n_which, npts, dim, dim] = d u_c / d X_d
        (None unless asked), cell [npts] the lexicographic id of the cell that answered (-1: outside, zeros), and how many
        points lie in no cell.  One id instead of a sequence drops the leading axis"""
        single = np.isscalar(which)
        ids = np.ascontiguousarray([which] if single else list(which), dtype=np.int32)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self.dim)
        npts = pts.shape[0]
        val = np.zeros((ids.size, npts, self.dim))
        grad = np.zeros((ids.size, npts, self.dim, self.dim)) if gradients else None
        cell = np.zeros(npts, dtype=np.int64)
        nout = C.c_int64(0)
        self._chk(lib().mi_evaluate_points(self.h, ids.size, ids.ctypes.data_as(C.POINTER(C.c_int)), npts, _dp(pts), _dp(val),
                                           _dp(grad) if gradients else None, cell.ctypes.data_as(C.POINTER(C.c_int64)),
                                           C.byref(nout)))
        if single:
            val, grad = val[0], (grad[0] if gradients else None)
        return val, grad, cell, int(nout.value)

    def evaluate_stress(self, xyz, model=STRESS_NEOHOOKE, kind=STRESS_AT_RAW, principal=False, directions=False):
        """the stress of the committed state at the points xyz [npts, dim] of the reference configuration (mi_evaluate_stress):
        dict(sigma [npts, ncomp], von_mises [npts], principal [npts, dim] descending, directions [npts, dim, dim] with row k the
        unit eigenvector of principal[k] (each None unless asked), cell [npts] (-1: outside, zeros), n_outside).  kind
        STRESS_AT_RAW: the answering element's own stress at the point; STRESS_AT_RECOVERED: stress_field(model) interpolated"""
        pts = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, self.dim)
        npts, ncomp = pts.shape[0], self.dim * (self.dim + 1) // 2
        sigma, vm = np.zeros((npts, ncomp)), np.zeros(npts)
        pr = np.zeros((npts, self.dim)) if principal else None
        dr = np.zeros((npts, self.dim, self.dim)) if directions else None
        cell = np.zeros(npts, dtype=np.int64)
        nout = C.c_int64(0)
        self._chk(lib().mi_evaluate_stress(self.h, int(model), int(kind), npts, _dp(pts), _dp(sigma), _dp(vm),
                                           _dp(pr) if principal else None, _dp(dr) if directions else None,
                                           cell.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(nout)))
        return dict(sigma=sigma, von_mises=vm, principal=pr, directions=dr, cell=cell, n_outside=int(nout.value))

    def principal_stress(self, sigma, directions=False):
        """(principal [n, dim] descending, directions [n, dim, dim] or None) of the symmetric tensors sigma [n, ncomp] in
        stress_field's component order (mi_principal_stress); row k of a tensor's directions is the unit eigenvector of its
        principal[k], its component of largest magnitude positive"""
        ncomp = self.dim * (self.dim + 1) // 2
        s = np.ascontiguousarray(sigma, dtype=np.float64).reshape(-1, ncomp)
        pr = np.zeros((s.shape[0], self.dim))
        dr = np.zeros((s.shape[0], self.dim, self.dim)) if directions else None
        self._chk(lib().mi_principal_stress(self.h, s.shape[0], _dp(s), _dp(pr), _dp(dr) if directions else None))
        return pr, dr

    def transfer_state_from(self, src):
        """this context's six state vectors V_U .. V_A_OLD := src's fields at this context's nodes, constrained dofs exactly 0
        (mi_state_transfer: evaluate on src at self.coords, device to device).  A node outside src's mesh: MiError, nothing
        written"""
        self._chk(lib().mi_state_transfer(self.h, src.h))

    def mass_apply(self, x, masked=False):
        """y = M x for the columns x [nrhs, n] (or one vector [n]): the unit-density consistent mass on the assembly's rule
        (mi_mass_apply).  masked: x read as 0 and y written 0 on constrained dofs"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        nrhs = 1 if x.ndim == 1 else x.shape[0]
        self._chk(lib().mi_mass_apply(self.h, nrhs, int(masked), _dp(x), _dp(y)))
        return y

    def mass_solve(self, b, masked=False, tol=1e-12, max_it=500, check=True):
        """(x, its, res[nrhs], rc) with M x = b for the columns b [nrhs, n] (or one vector [n]) by the device's Jacobi-PCG
        (mi_mass_solve).  Not converged: MiError with code MI_ENOCONV_LIN whose .partial is that tuple; check=False returns it"""
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros_like(b)
        nrhs = 1 if b.ndim == 1 else b.shape[0]
        its, res = C.c_int(0), np.zeros(max(nrhs, 1))
        rc = lib().mi_mass_solve(self.h, nrhs, int(masked), _dp(b), _dp(x), float(tol), int(max_it), C.byref(its), _dp(res))
        out = (x, its.value, res[:nrhs], rc)
        if rc == MI_ENOCONV_LIN:
            if check:
                raise MiError(rc, lib().mi_last_error(self.h).decode(), partial=out)
            return out
        self._chk(rc)
        return out

    def project_load(self, src, which, sub=1):
        """b [n_which, n] (one id: [n]): the load of src's state vectors `which` against this context's test functions on the
        composite rule sub^dim x QGauss(p + 2) per cell (mi_project_load); every dof, nothing masked"""
        single = np.isscalar(which)
        ids = np.ascontiguousarray([which] if single else list(which), dtype=np.int32)
        b = np.zeros((ids.size, self.n))
        self._chk(lib().mi_project_load(self.h, src.h, ids.size, ids.ctypes.data_as(C.POINTER(C.c_int)), int(sub), _dp(b)))
        return b[0] if single else b

    def project_state_from(self, src, sub=1, tol=1e-12, max_it=500):
        """this context's six state vectors V_U .. V_A_OLD := the L2 projection of src's fields onto this context's space,
        constrained dofs exactly 0 (mi_state_project).  Returns dict(its, sub, n_points, res, src_sq[6], dst_sq[6]); on an
        error -- a point outside src's mesh, no convergence -- MiError and nothing is written"""
        info = ProjectInfo()
        self._chk(lib().mi_state_project(self.h, src.h, int(sub), float(tol), int(max_it), C.byref(info)))
        return dict(its=info.its, sub=info.sub, n_points=int(info.n_points), res=info.res, src_sq=np.array(info.src_sq),
                    dst_sq=np.array(info.dst_sq))

    def state_save(self):
        self._chk(lib().mi_state_save(self.h))

    def state_restore(self):
        self._chk(lib().mi_state_restore(self.h))

    def csr(self):
        import scipy.sparse as sp
        rp = np.zeros(self.n + 1, dtype=np.int64)
        col = np.zeros(self.nnz, dtype=np.int32)
        val = np.zeros(self.nnz)
        self._chk(lib().mi_matrix_get_csr(self.h, rp.ctypes.data_as(C.POINTER(C.c_int64)),
                                          col.ctypes.data_as(C.POINTER(C.c_int32)), _dp(val)))
        return sp.csr_matrix((val, col, rp), shape=(self.n, self.n))

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        self._chk(lib().mi_spmv(self.h, _dp(x), _dp(y)))
        return y

    def diagonal_blocks(self):
        """[n_nodes, dim, dim]: the diagonal block of every node of the current tangent"""
        b = np.zeros((self.nnodes, self.dim, self.dim))
        self._chk(lib().mi_get_diagonal_blocks(self.h, _dp(b)))
        return b

    def spmm(self, X, out=None):
        """Y [n, nv] with Y[:, j] = K X[:, j] through the block product where the context is eligible (mi_spmm), else column by
        column; out [n, nv]: its values stand where nobody computes a row"""
        xt = np.ascontiguousarray(np.asarray(X, dtype=np.float64).T)
        yt = np.zeros_like(xt) if out is None else np.ascontiguousarray(np.asarray(out, dtype=np.float64).T)
        self._chk(lib().mi_spmm(self.h, xt.shape[0], _dp(xt), _dp(yt)))
        return yt.T.copy()

    # ---- the multigrid hierarchy as the last linear solve left it, read-only (tests)
    def mg_n_levels(self):
        return lib().mi_mg_n_levels(self.h)

    def mg_level_describe(self, level):
        d = MgLevelDesc()
        self._chk(lib().mi_mg_level_describe(self.h, level, C.byref(d)))
        return self._level_desc(d)

    def mg_level_context(self, level):
        h = C.c_void_p()
        self._chk(lib().mi_mg_level_context(self.h, level, C.byref(h)))
        return LevelView(self, h)

    def _level_desc(self, d):
        return dict(degree=d.degree, reps=tuple(d.reps)[:self.dim], n_dofs=d.n_dofs, lmax=d.lmax,
                    interval_ratio=d.interval_ratio, smoother_degree=d.smoother_degree, exact_solve=d.exact_solve,
                    distributed=d.distributed)

    # ---- the linear model's own hierarchy (tuning key "linear_precond" 1), complete after linear_setup
    def linear_mg_n_levels(self):
        return lib().mi_linear_mg_n_levels(self.h)

    def linear_mg_level_describe(self, level):
        d = MgLevelDesc()
        self._chk(lib().mi_linear_mg_level_describe(self.h, level, C.byref(d)))
        return self._level_desc(d)

    def linear_mg_level_context(self, level):
        h = C.c_void_p()
        self._chk(lib().mi_linear_mg_level_context(self.h, level, C.byref(h)))
        return LevelView(self, h)

    # ---- linear model (mi_linear_setup / mi_linear_step); the operators follow the tuning key "linear_operator"
    def linear_setup(self, theta):
        self._chk(lib().mi_linear_setup(self.h, float(theta)))

    def linear_step(self, data_consistent, abs_tol, max_it=None):
        """one step; returns (CG iterations, residual)"""
        its, res = C.c_int(0), C.c_double(0)
        self._chk(lib().mi_linear_step(self.h, int(data_consistent), abs_tol, self.n * 10 if max_it is None else max_it,
                                       C.byref(its), C.byref(res)))
        return its.value, res.value

    def linear_energy(self):
        """1/2 u.K u, 1/2 v.M v and -u.f_body of the linear model, through the products of the current set-up"""
        e = EnergyInfo()
        self._chk(lib().mi_linear_energy(self.h, C.byref(e)))
        return dict(strain=e.strain, kinetic=e.kinetic, body=e.body)

    def linear_modes(self, n_modes, tol=1e-8, max_it=1000, want_modes=True):
        """the n_modes lowest eigenpairs of K phi = lam M phi on the free dofs (mi_linear_modes): dict(lam[n_modes],
        modes[n_modes, n] or None, residual[n_modes], its).  Not converged within max_it: MiError with code MI_ENOCONV_LIN whose
        .partial is that dict"""
        lam, res, its = np.zeros(n_modes), np.zeros(n_modes), C.c_int(0)
        modes = np.zeros((n_modes, self.n)) if want_modes else None
        rc = lib().mi_linear_modes(self.h, int(n_modes), float(tol), int(max_it), _dp(lam), _dp(modes) if want_modes else None,
                                   _dp(res), C.byref(its))
        out = dict(lam=lam, modes=modes, residual=res, its=its.value)
        if rc == MI_ENOCONV_LIN:
            raise MiError(rc, lib().mi_last_error(self.h).decode(), partial=out)
        self._chk(rc)
        return out

    def tangent_modes(self, n_modes, tol=1e-8, max_it=1000, want_modes=True):
        """the n_modes algebraically smallest eigenpairs of K_T(u) phi = lam rho M phi on the free dofs, K_T the nonlinear model's
        tangent stiffness at the committed state V_U (mi_tangent_modes): dict(lam[n_modes], modes[n_modes, n] or None,
        residual[n_modes], its).  A negative lam is a buckled state.  Not converged within max_it: MiError with code
        MI_ENOCONV_LIN whose .partial is that dict"""
        lam, res, its = np.zeros(n_modes), np.zeros(n_modes), C.c_int(0)
        modes = np.zeros((n_modes, self.n)) if want_modes else None
        rc = lib().mi_tangent_modes(self.h, int(n_modes), float(tol), int(max_it), _dp(lam), _dp(modes) if want_modes else None,
                                    _dp(res), C.byref(its))
        out = dict(lam=lam, modes=modes, residual=res, its=its.value)
        if rc == MI_ENOCONV_LIN:
            raise MiError(rc, lib().mi_last_error(self.h).decode(), partial=out)
        self._chk(rc)
        return out

    # ---- explicit central differences of the nonlinear model (mi_explicit_*)
    def explicit_setup(self, dt, init_acceleration=True):
        """the lumped masses and the step of the following explicit_run calls; init_acceleration: V_A, V_A_OLD := minv F(u) of the
        committed state (V_DELTA := 0), else the state stays as it is"""
        self._chk(lib().mi_explicit_setup(self.h, float(dt), int(bool(init_acceleration))))

    def explicit_run(self, n, check=True):
        """n explicit steps on the device, one read-back: dict(rc, steps_done, inverted_step (-1: none), dt, kinetic_lumped).  A step
        whose force pass finds det F <= 0 ends the run: MiError (code MI_EINVAL, .partial that dict), or with check=False the dict"""
        info = ExplicitInfo()
        rc = lib().mi_explicit_run(self.h, int(n), C.byref(info))
        out = dict(rc=rc, steps_done=info.steps_done, inverted_step=info.inverted_step, dt=info.dt, kinetic_lumped=info.kinetic_lumped)
        if rc != MI_OK and check:
            raise MiError(rc, lib().mi_last_error(self.h).decode(), partial=out)
        return out

    def explicit_mass(self):
        """the lumped masses [n]: rho times the row sums of the consistent mass of mass_apply"""
        m = np.zeros(self.n)
        self._chk(lib().mi_explicit_get_mass(self.h, _dp(m)))
        return m

    def explicit_stable_dt(self, krylov_steps=40):
        """(lambda_max, dt_crit): the largest Ritz value of krylov_steps Lanczos steps for K_T phi = lambda M_L phi at the committed
        state -- a lower bound of lambda_max -- and 2 / sqrt of it; multiply dt_crit by a safety factor"""
        lam, dt = C.c_double(0), C.c_double(0)
        self._chk(lib().mi_explicit_stable_dt(self.h, int(krylov_steps), C.byref(lam), C.byref(dt)))
        return lam.value, dt.value

    def linear_apply(self, which, x):
        """y = K x (0), M x (1), A x (2) through the device kernels of the current set-up; 3: one V-cycle of its multigrid"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        self._chk(lib().mi_linear_apply(self.h, which, _dp(x), _dp(y)))
        return y

    def linear_csr(self, which):
        """K (0), M (1) or the constrained stepping matrix (2) of an assembled set-up"""
        import scipy.sparse as sp
        rp = np.zeros(self.n + 1, dtype=np.int64)
        col = np.zeros(self.nnz, dtype=np.int32)
        val = np.zeros(self.nnz)
        self._chk(lib().mi_linear_matrix_get_csr(self.h, which, rp.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 col.ctypes.data_as(C.POINTER(C.c_int32)), _dp(val)))
        return sp.csr_matrix((val, col, rp), shape=(self.n, self.n))

    def linear_diagonal(self):
        """the Jacobi diagonal of the stepping matrix in use"""
        d = np.zeros(self.n)
        self._chk(lib().mi_linear_get_diagonal(self.h, _dp(d)))
        return d

    def linear_diagonal_blocks(self):
        """[n_nodes, dim, dim]: the node blocks of the stepping matrix in use (the smoother's D under "linear_precond" 1)"""
        b = np.zeros((self.nnodes, self.dim, self.dim))
        self._chk(lib().mi_linear_get_diagonal_blocks(self.h, _dp(b)))
        return b

    def set_profiling(self, on=True):
        self._chk(lib().mi_set_profiling(self.h, int(on)))

    def set_tuning(self, key, value):
        self._chk(lib().mi_set_tuning(self.h, key.encode(), int(value)))

    def get_tuning(self, key):
        v = C.c_int(0)
        self._chk(lib().mi_get_tuning(self.h, key.encode(), C.byref(v)))
        return v.value

    def reset_timings(self):
        self._chk(lib().mi_reset_timings(self.h))

    def timings(self):
        t = Timings()
        self._chk(lib().mi_get_timings(self.h, C.byref(t)))
        return {TIMING_NAMES[i]: (t.ms[i], t.count[i]) for i in range(T_COUNT)}

    def bench_spmv(self, reps=20):
        ms = C.c_double(0)
        self._chk(lib().mi_bench_spmv(self.h, reps, C.byref(ms)))
        return ms.value

    def bench_spmm(self, nv, reps=10, rounds=5):
        """(ms_block[rounds], ms_single[rounds]): the block product on nv columns against nv single products, alternated"""
        a, b = np.zeros(rounds), np.zeros(rounds)
        self._chk(lib().mi_bench_spmm(self.h, int(nv), int(reps), int(rounds), _dp(a), _dp(b)))
        return a, b

    def bench_assemble(self, reps=3):
        ms = C.c_double(0)
        self._chk(lib().mi_bench_assemble(self.h, reps, C.byref(ms)))
        return ms.value
