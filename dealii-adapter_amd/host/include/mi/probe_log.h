// mi::ProbeLog -- the executables' MI_PROBES=<file>: displacement and velocity at arbitrary points of the structure, one row per
// completed time window in probes.log in the working directory (beside the coupling partner's displacement log).
//
// The file lists one point of the REFERENCE configuration per line, dim numbers each; empty lines and lines that start with '#'
// are skipped.  A row of probes.log: the time, then for every probe in the file's order its displacement (dim numbers) and its
// velocity (dim numbers), 17 significant digits -- the finite-element fields themselves (Device::evaluate_points), so a probe
// that is no node (FSI3's point A, the middle of the flap's end: a cell centre of the 18 x 3 flap) needs no post-processing.
// MI_PROBES_STRESS=raw|recovered appends to every probe's columns its stress (dim (dim + 1) / 2 numbers, xx yy zz xy xz yz or
// xx yy xy) and von Mises stress (Device::evaluate_stress: the element's own stress at the point, or the recovered nodal field
// interpolated; the linear executable's model is MI_STRESS_LINEAR, the nonlinear one's MI_STRESS_NEOHOOKE; the header line says
// which); any other value is a start-up error, and without the variable the file is what it was.
// A probe outside the mesh is a start-up error that names the point.  On a team the library evaluates no points: said once, no
// log is written.  Without the variable nothing is read, written or printed.
#pragma once
#include <cstdlib>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include <mi/device_vector.h>

namespace mi
{
  class ProbeLog
  {
  public:
    // which_u, which_v: the model's displacement and velocity (MI_V_* / MI_L_*); stress_model: MI_STRESS_NEOHOOKE / MI_STRESS_LINEAR
    void open(const Device &dev, int dim, int which_u, int which_v, int stress_model)
    {
      const char *file = std::getenv("MI_PROBES");
      if (!file || !*file)
        return;
      if (const char *kind = std::getenv("MI_PROBES_STRESS"))
        {
          if (std::string(kind) == "raw")
            stress_kind_ = MI_STRESS_AT_RAW;
          else if (std::string(kind) == "recovered")
            stress_kind_ = MI_STRESS_AT_RECOVERED;
          else
            throw std::runtime_error(std::string("MI_PROBES_STRESS: '") + kind + "' is neither raw nor recovered");
          stress_model_ = stress_model;
        }
      std::ifstream in(file);
      if (!in)
        throw std::runtime_error(std::string("MI_PROBES: cannot read ") + file);
      std::string line;
      for (int no = 1; std::getline(in, line); ++no)
        {
          if (line.find_first_not_of(" \t\r") == std::string::npos || line[line.find_first_not_of(" \t\r")] == '#')
            continue;
          std::istringstream s(line);
          double             x[3] = {0, 0, 0};
          for (int d = 0; d < dim; ++d)
            if (!(s >> x[d]))
              throw std::runtime_error(std::string("MI_PROBES: line ") + std::to_string(no) + " of " + file + " does not hold " +
                                       std::to_string(dim) + " numbers");
          xyz_.insert(xyz_.end(), x, x + dim);
        }
      dev_ = &dev, dim_ = dim, which_ = {which_u, which_v};
      std::vector<double>  values;
      std::vector<int64_t> cells;
      const int64_t        outside = dev.evaluate_points(which_, dim, xyz_, values, &cells);
      if (outside < 0)
        {
          std::cout << "MI_PROBES ignored: mi_evaluate_points runs on one slab only, no probes are written on a team" << std::endl;
          xyz_.clear();
          return;
        }
      for (size_t k = 0; outside > 0 && k < cells.size(); ++k)
        if (cells[k] < 0)
          {
            std::ostringstream msg;
            msg << std::setprecision(17) << "MI_PROBES: probe " << k + 1 << " of " << file << " at (";
            for (int d = 0; d < dim; ++d)
              msg << (d ? ", " : "") << xyz_[k * size_t(dim) + size_t(d)];
            msg << ") lies outside the mesh";
            throw std::runtime_error(msg.str());
          }
      out_.open("probes.log");
      if (stress_kind_ < 0)
        out_ << "# t, then displacement and velocity (" << dim << " numbers each) of each of " << cells.size() << " probes of " << file
             << ", per completed time window\n";
      else
        out_ << "# t, then displacement and velocity (" << dim << " numbers each), the "
             << (stress_kind_ == MI_STRESS_AT_RAW ? "raw" : "recovered") << " stress of model " << stress_model_
             << (stress_model_ == MI_STRESS_LINEAR ? " (linear)" : " (neo-Hookean Cauchy)") << " (" << dim * (dim + 1) / 2
             << " numbers: " << (dim == 3 ? "xx yy zz xy xz yz" : "xx yy xy") << ") and its von Mises stress of each of "
             << cells.size() << " probes of " << file << ", per completed time window\n";
    }
    bool active() const { return out_.is_open(); }
    void write(double t)
    {
      if (!active())
        return;
      std::vector<double> values;
      dev_->evaluate_points(which_, dim_, xyz_, values);
      const size_t npts = xyz_.size() / size_t(dim_), d = size_t(dim_), ncomp = d * (d + 1) / 2;
      std::vector<double> sigma, von_mises;
      if (stress_kind_ >= 0)
        dev_->evaluate_stress(stress_model_, stress_kind_, dim_, xyz_, sigma, von_mises);
      out_ << std::setprecision(17) << t;
      for (size_t k = 0; k < npts; ++k)
        {
          for (size_t w = 0; w < 2; ++w)
            for (size_t c = 0; c < d; ++c)
              out_ << ' ' << values[(w * npts + k) * d + c];
          if (stress_kind_ >= 0)
            {
              for (size_t c = 0; c < ncomp; ++c)
                out_ << ' ' << sigma[k * ncomp + c];
              out_ << ' ' << von_mises[k];
            }
        }
      out_ << '\n' << std::flush;
    }

  private:
    const Device       *dev_ = nullptr;
    int                 dim_ = 0;
    int                 stress_kind_ = -1, stress_model_ = 0; // MI_PROBES_STRESS=raw|recovered: MI_STRESS_AT_*, or -1 without it
    std::vector<int>    which_;
    std::vector<double> xyz_;
    std::ofstream       out_;
  };
} // namespace mi
