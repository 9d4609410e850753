// mi::Device / mi::Vector -- thin C++ RAII layer over the C-ABI (include/mi_elasticity.h) for the host solvers.
//
// mi::Vector plays the role of the reference's VectorType (BlockVector<double>): a *handle* to a
// device-resident global vector.  Copy-assignment copies device-to-device, so the Adapter's checkpoint code
// (`old_state_data[i] = *state_variables[i]`, adapter.h:457-460) keeps its shape while the data never leaves HBM.
#pragma once
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "mi_elasticity.h"
#include "rank_identity.h"

namespace mi
{
  // (decomposition of the executables: mi/rank_identity.h)
  struct Error : std::runtime_error
  {
    int code;
    Error(int c, const std::string &what)
      : std::runtime_error(what)
      , code(c)
    {}
  };

  class Device
  {
  public:
    Device(const mi_mesh_desc &mesh, const mi_material_desc &mat, const mi_newmark_desc &nm, int device_id = 0)
    {
      mi_comm_desc  comm;
      mi_comm_desc *use = nullptr;
      std::memset(&comm, 0, sizeof(comm));
      const int world = host_world_size();
      if (world > 1)
        {
          comm.rank = host_rank();
          comm.size = world;
          if (comm.rank < 0 || comm.rank >= world)
            throw Error(MI_EINVAL, "MI_RANK outside [0, MI_WORLD_SIZE)");
          if (thread_identity().world > 0) // rank threads of one process (tests): id and device come with the identity
            {
              if (!thread_identity().uid)
                throw Error(MI_EINVAL, "rank thread without an RCCL id");
              std::memcpy(uid_, thread_identity().uid, 128);
              device_id = thread_identity().device;
            }
          else
            {
              const char *file = std::getenv("MI_UID_FILE");
              if (!file)
                throw Error(MI_EINVAL, "MI_WORLD_SIZE > 1 needs MI_UID_FILE (see tools/launch_elasticity.py)");
              exchange_unique_id(file, comm.rank, uid_);
              if (const char *e = std::getenv("MI_LOCAL_RANK"))
                device_id = std::atoi(e);
              else
                device_id = comm.rank;
            }
          comm.nccl_unique_id = uid_;
          use                 = &comm;
        }
      else if (const char *e = std::getenv("MI_SLABS"))
        {
          if (std::atoi(e) > 1)
            {
              comm.rank = -1; // all slabs in this process
              comm.size = std::atoi(e);
              use       = &comm;
            }
        }
      const int rc = mi_ctx_create(&mesh, &mat, &nm, device_id, use, &ctx_);
      if (rc != MI_OK)
        throw Error(rc, std::string("mi_ctx_create: ") + mi_last_error(nullptr));
    }
    ~Device() { mi_ctx_destroy(ctx_); }
    Device(const Device &)            = delete;
    Device &operator=(const Device &) = delete;

    mi_ctx *ctx() const { return ctx_; }
    // nodal stress field of the committed state (mi_stress_field; model MI_STRESS_NEOHOOKE / MI_STRESS_LINEAR): sigma
    // [n_nodes][dim (dim + 1) / 2] and von Mises [n_nodes] in the reference's node order.  false on an RCCL team, where the
    // library provides none (one process only); any other failure throws
    bool stress_field(int model, int dim, std::vector<double> &sigma, std::vector<double> &von_mises) const
    {
      int team = 1, rccl = 0;
      check(mi_comm_info(ctx_, &team, &rccl), "mi_comm_info");
      if (rccl > 0)
        return false;
      const size_t nn = size_t(mi_n_nodes(ctx_));
      sigma.assign(nn * size_t(dim * (dim + 1) / 2), 0.0);
      von_mises.assign(nn, 0.0);
      check(mi_stress_field(ctx_, model, sigma.data(), von_mises.data(), nullptr), "mi_stress_field");
      return true;
    }
    // error indicator of that stress field (mi_stress_error): the totals into info, eta_K [n_cells] in lexicographic cell order
    // into eta_cell where wanted.  false on a team (emulated slabs or RCCL), where the library provides none (one slab only);
    // any other failure throws
    bool stress_error(int model, mi_stress_error_info &info, std::vector<double> *eta_cell = nullptr) const
    {
      int team = 1, rccl = 0;
      check(mi_comm_info(ctx_, &team, &rccl), "mi_comm_info");
      if (team > 1 || rccl > 0)
        return false;
      if (eta_cell)
        eta_cell->assign(size_t(mi_n_cells(ctx_)), 0.0);
      check(mi_stress_error(ctx_, model, &info, eta_cell ? eta_cell->data() : nullptr, nullptr), "mi_stress_error");
      return true;
    }
    // support reactions and load resultants of the committed state (mi_reactions), moments about the origin: the resultants
    // into info, the out-of-balance force on every dof [n_dofs] into forces where wanted.  false on a team (emulated slabs or
    // RCCL), where the library provides none (one slab only); any other failure throws
    bool reactions(int model, mi_reaction_info &info, std::vector<double> *forces = nullptr) const
    {
      int team = 1, rccl = 0;
      check(mi_comm_info(ctx_, &team, &rccl), "mi_comm_info");
      if (team > 1 || rccl > 0)
        return false;
      if (forces)
        forces->assign(size_t(mi_n_dofs(ctx_)), 0.0);
      check(mi_reactions(ctx_, model, nullptr, &info, forces ? forces->data() : nullptr, nullptr), "mi_reactions");
      return true;
    }
    // the fields at npts points of the reference configuration (mi_evaluate_points): values [n_which][npts][dim] of the state
    // vectors which[], cells [npts] (the lexicographic id of the cell that answered, -1: outside) where wanted; returns the number
    // of points in no cell, or -1 on a team (emulated slabs or RCCL), where the library provides none (one slab only); any other
    // failure throws
    int64_t evaluate_points(const std::vector<int> &which, int dim, const std::vector<double> &xyz, std::vector<double> &values,
                            std::vector<int64_t> *cells = nullptr) const
    {
      int team = 1, rccl = 0;
      check(mi_comm_info(ctx_, &team, &rccl), "mi_comm_info");
      if (team > 1 || rccl > 0)
        return -1;
      const size_t npts = xyz.size() / size_t(dim);
      values.assign(which.size() * npts * size_t(dim), 0.0);
      if (cells)
        cells->assign(npts, -1);
      int64_t n_outside = 0;
      check(mi_evaluate_points(ctx_, int(which.size()), which.data(), int64_t(npts), xyz.data(), values.data(), nullptr,
                               cells ? cells->data() : nullptr, &n_outside),
            "mi_evaluate_points");
      return n_outside;
    }
    // the stress of the committed state at npts points of the reference configuration (mi_evaluate_stress; model as
    // stress_field, kind MI_STRESS_AT_RAW / MI_STRESS_AT_RECOVERED): sigma [npts][dim (dim + 1) / 2] and von Mises [npts]; returns
    // the number of points in no cell (zeros there), or -1 on a team (emulated slabs or RCCL), where the library provides none
    // (one slab only); any other failure throws
    int64_t evaluate_stress(int model, int kind, int dim, const std::vector<double> &xyz, std::vector<double> &sigma,
                            std::vector<double> &von_mises) const
    {
      int team = 1, rccl = 0;
      check(mi_comm_info(ctx_, &team, &rccl), "mi_comm_info");
      if (team > 1 || rccl > 0)
        return -1;
      const size_t npts = xyz.size() / size_t(dim);
      sigma.assign(npts * size_t(dim * (dim + 1) / 2), 0.0);
      von_mises.assign(npts, 0.0);
      int64_t n_outside = 0;
      check(mi_evaluate_stress(ctx_, model, kind, int64_t(npts), xyz.data(), sigma.data(), von_mises.data(), nullptr, nullptr, nullptr,
                               &n_outside),
            "mi_evaluate_stress");
      return n_outside;
    }
    // principal values [n][dim], descending, of the n tensors sigma [n][dim (dim + 1) / 2] (mi_principal_stress)
    void principal_stress(int dim, const std::vector<double> &sigma, std::vector<double> &principal) const
    {
      const size_t n = sigma.size() / size_t(dim * (dim + 1) / 2);
      principal.assign(n * size_t(dim), 0.0);
      check(mi_principal_stress(ctx_, int64_t(n), sigma.data(), principal.data(), nullptr), "mi_principal_stress");
    }
    // this device's six state vectors := the L2 projection of src's fields onto its space (mi_state_project: the load on the
    // composite rule sub^dim x QGauss(p + 2) per cell, the consistent-mass solve on the free dofs, device to device); the
    // iteration count, residual and the two integrals of |w|^2 into info where wanted.  false on a team (emulated slabs or
    // RCCL) on either side, where the library provides none (one slab only); any other failure throws and leaves this device
    // unchanged
    bool project_state(const Device &src, int sub = 1, double tol = 1e-12, int max_it = 500, mi_project_info *info = nullptr)
    {
      for (const mi_ctx *c : {ctx_, src.ctx_})
        {
          int team = 1, rccl = 0;
          check(mi_comm_info(c, &team, &rccl), "mi_comm_info");
          if (team > 1 || rccl > 0)
            return false;
        }
      check(mi_state_project(ctx_, src.ctx_, sub, tol, max_it, info), "mi_state_project");
      return true;
    }
    // the n_modes algebraically smallest eigenvalues of K_T(u) phi = lambda rho M phi at the committed state (mi_tangent_modes, no
    // mode shapes): lambda and residual [n_modes], the iteration count.  Returns MI_OK or MI_ENOCONV_LIN (the best pairs are
    // written); -1 on a team (emulated slabs or RCCL), where the library provides none (one slab only); any other failure throws
    int tangent_modes(int n_modes, std::vector<double> &lambda, std::vector<double> &residual, int &its, double tol = 1e-8,
                      int max_it = 1000)
    {
      int team = 1, rccl = 0;
      check(mi_comm_info(ctx_, &team, &rccl), "mi_comm_info");
      if (team > 1 || rccl > 0)
        return -1;
      lambda.assign(size_t(n_modes > 0 ? n_modes : 0), 0.0);
      residual.assign(lambda.size(), 0.0);
      const int rc = mi_tangent_modes(ctx_, n_modes, tol, max_it, lambda.data(), nullptr, residual.data(), &its);
      if (rc != MI_ENOCONV_LIN)
        check(rc, "mi_tangent_modes");
      return rc;
    }
    // explicit central differences of the nonlinear model (mi_explicit_setup / mi_explicit_run / mi_explicit_stable_dt; one slab
    // only: on a team the library's refusal is thrown).  explicit_run: a step whose force pass finds det F <= 0 ends the run, the
    // library's message ("inverted element ... at explicit step k") is thrown with info filled
    void explicit_setup(double dt, bool init_acceleration) { check(mi_explicit_setup(ctx_, dt, init_acceleration ? 1 : 0), "mi_explicit_setup"); }
    void explicit_run(int n_steps, mi_explicit_info &info) { check(mi_explicit_run(ctx_, n_steps, &info), "mi_explicit_run"); }
    void explicit_stable_dt(double &lambda_max, double &dt_crit, int krylov_steps = 40)
    {
      check(mi_explicit_stable_dt(ctx_, krylov_steps, &lambda_max, &dt_crit), "mi_explicit_stable_dt");
    }
    void    check(int rc, const char *what) const
    {
      if (rc != MI_OK)
        throw Error(rc, std::string(what) + ": " + mi_last_error(ctx_));
    }

  private:
    // rank 0 writes the 128-byte RCCL id (to a temporary name, then renamed: never seen half written), the others
    // poll for it for up to two minutes
    static void exchange_unique_id(const std::string &file, int rank, unsigned char *uid)
    {
      const size_t nb = 128;
      if (rank == 0)
        {
          if (mi_comm_unique_id(uid) != MI_OK)
            throw Error(MI_EINVAL, std::string("mi_comm_unique_id: ") + mi_last_error(nullptr));
          const std::string tmp = file + ".tmp";
          std::FILE        *f   = std::fopen(tmp.c_str(), "wb");
          if (!f || std::fwrite(uid, 1, nb, f) != nb)
            throw Error(MI_EINVAL, "cannot write " + tmp);
          std::fclose(f);
          if (std::rename(tmp.c_str(), file.c_str()))
            throw Error(MI_EINVAL, "cannot rename " + tmp);
          return;
        }
      for (int tries = 0; tries < 2400; ++tries)
        {
          if (std::FILE *f = std::fopen(file.c_str(), "rb"))
            {
              const size_t got = std::fread(uid, 1, nb, f);
              std::fclose(f);
              if (got == nb)
                return;
            }
          std::this_thread::sleep_for(std::chrono::milliseconds(50));
        }
      throw Error(MI_EINVAL, "no RCCL id in " + file + " after two minutes (is rank 0 running?)");
    }
    mi_ctx       *ctx_ = nullptr;
    unsigned char uid_[128] = {0};
  };

  class Vector
  {
  public:
    Vector() = default; // empty snapshot, storage created on first assignment
    Vector(const Device &dev, int which)
      : dev_(&dev)
      , which_(which)
    {}
    Vector(const Vector &o) { *this = o; }
    Vector(Vector &&o) noexcept
      : dev_(o.dev_)
      , which_(o.which_)
      , snap_(o.snap_)
    {
      o.snap_ = nullptr;
    }
    Vector &operator=(Vector &&o) noexcept
    {
      if (this != &o)
        {
          release();
          dev_    = o.dev_;
          which_  = o.which_;
          snap_   = o.snap_;
          o.snap_ = nullptr;
        }
      return *this;
    }
    ~Vector() { release(); }

    // make this handle refer to state vector `which` of the device context (no data is copied)
    void bind(const Device &dev, int which)
    {
      release();
      dev_   = &dev;
      which_ = which;
    }

    Vector &operator=(const Vector &o)
    {
      if (this == &o || !o.dev_)
        return *this;
      if (!dev_)
        dev_ = o.dev_;
      if (which_ < 0 && !snap_)
        dev_->check(mi_snapshot_create(dev_->ctx(), &snap_), "mi_snapshot_create");
      if (which_ >= 0 && o.which_ < 0) // state vector := snapshot
        dev_->check(mi_snapshot_load(dev_->ctx(), o.snap_, which_), "mi_snapshot_load");
      else if (which_ < 0 && o.which_ >= 0) // snapshot := state vector
        dev_->check(mi_snapshot_store(dev_->ctx(), snap_, o.which_), "mi_snapshot_store");
      else
        throw std::logic_error("mi::Vector: only state <-> snapshot assignments are supported");
      return *this;
    }

    bool is_state() const { return which_ >= 0; }
    int  id() const { return which_; }
    const Device &device() const { return *dev_; }

    // interface-sized transfers (format_deal_to_precice / format_precice_to_deal, adapter.h:389-443)
    void gather_interface(std::vector<double> &out, int n_nodes) const
    {
      if (which_ != MI_V_TOTAL_DISPLACEMENT)
        throw std::logic_error("only the total displacement is written to the coupling interface");
      dev_->check(mi_get_interface_displacement(dev_->ctx(), n_nodes, out.data()), "mi_get_interface_displacement");
    }
    void scatter_interface(const std::vector<double> &in, int n_nodes)
    {
      if (which_ != MI_V_EXTERNAL_STRESS)
        throw std::logic_error("coupling data is read into the external stress vector");
      dev_->check(mi_set_interface_traction(dev_->ctx(), n_nodes, in.data()), "mi_set_interface_traction");
    }

  private:
    void release()
    {
      if (snap_ && dev_)
        mi_snapshot_destroy(dev_->ctx(), snap_);
      snap_ = nullptr;
    }
    const Device *dev_   = nullptr;
    int           which_ = -1;
    mi_snapshot  *snap_  = nullptr;
  };
} // namespace mi
