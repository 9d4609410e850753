// mi::ReactionLog -- the executables' MI_REACTIONS=1: what the supports carry and whether the structure is in balance with its
// loads, one row per completed time window in reactions.log in the working directory (beside the coupling partner's displacement
// log).
//
// A row: the time, then the reaction force (3 numbers) and its moment about the origin (3), the load, inertia and body-force
// resultants (3 each) and max_unbalanced, 17 significant digits -- mi_reactions of the step's committed state
// (Device::reactions).  2D: a force's z entry and a moment's x and y entries are 0.  Every row satisfies
// reaction + unbalanced = inertia - body - load; with the solver converged, unbalanced is its residual.  A header line names the
// columns.  On a team the library forms no reactions: said once, no log is written.  Without the variable nothing is written or
// printed.
#pragma once
#include <cstdlib>
#include <fstream>
#include <iomanip>
#include <iostream>

#include <mi/device_vector.h>

namespace mi
{
  class ReactionLog
  {
  public:
    // model: MI_STRESS_NEOHOOKE (the Newmark model's terms) / MI_STRESS_LINEAR (the theta scheme's)
    void open(const Device &dev, int model)
    {
      const char *e = std::getenv("MI_REACTIONS");
      if (!e || std::atoi(e) == 0)
        return;
      mi_reaction_info info{};
      if (!dev.reactions(model, info))
        {
          std::cout << "MI_REACTIONS ignored: mi_reactions runs on one slab only, no reactions are written on a team" << std::endl;
          return;
        }
      dev_ = &dev, model_ = model;
      out_.open("reactions.log");
      out_ << "# t reaction_x reaction_y reaction_z reaction_moment_x reaction_moment_y reaction_moment_z load_x load_y load_z "
              "inertia_x inertia_y inertia_z body_x body_y body_z max_unbalanced  (moments about the origin; per completed time window)\n";
    }
    bool active() const { return out_.is_open(); }
    void write(double t)
    {
      if (!active())
        return;
      mi_reaction_info info{};
      if (!dev_->reactions(model_, info)) // (a team: open() has said so and opened no log)
        return;
      out_ << std::setprecision(17) << t;
      for (const double *v : {info.reaction, info.reaction_moment, info.load, info.inertia, info.body})
        for (int c = 0; c < 3; ++c)
          out_ << ' ' << v[c];
      out_ << ' ' << info.max_unbalanced << '\n' << std::flush;
    }

  private:
    const Device *dev_   = nullptr;
    int           model_ = 0;
    std::ofstream out_;
  };
} // namespace mi
