// Fused routes of the ADMM sweep.
//
// A driver (admm.cc) whose problem has a structure that hand-written kernels sweep in one pass
// over the data matrix hands its sweep to a FusedRoute: the route owns the recognised structure,
// the iterate state (the driver's containers become views of it), the kernels' argument records
// and every knob of its own.  The driver keeps the iteration, the stopping rule and the capture
// of a batch of sweeps into a hipGraph; without a route it runs the reference's operator sweep.
#pragma once

#include <memory>
#include <vector>

#include "block.h"
#include "prox.h"

namespace eps {

class FusedRoute {
 public:
  virtual ~FusedRoute() {}
  virtual void Sweep() = 0;

  // A route with a residual check of its own splits it into device work that is only enqueued
  // (LaunchNorms: its scalars into the next slots of the Runtime) and, after the fetch, the host
  // part; a route without one leaves the driver's generic check to run on the views.
  virtual bool HasCheck() const { return false; }
  virtual bool PipelineChecks() const { return false; }  // Solver::PipelinedChecks for this route
  virtual void LaunchNorms() {}
  struct Check {
    double r = 0, s = 0;  // ||sum_i A x_i - b||, ||A_i^T (y - y_prev)|| (the driver applies rho)
    double max_norm = 0;  // max_i ||A x_i||
    double atu = 0;       // ||A^T u||
  };
  virtual Check FinishCheck() { return Check(); }
  virtual void SaveSnapshot() {}
  virtual void RestoreSnapshot() {}

  // Every launch of a sweep works on fixed buffers and none is a collective call: a batch of
  // sweeps may be captured into a hipGraph; CaptureByDefault: the route gains from it.
  virtual bool Capturable() const { return false; }
  virtual bool CaptureByDefault() const { return false; }
};

// What recognition reads of a driver and re-points at the route's state.
struct MultiBlockParts {
  int num_constraints;
  const BlockMatrix& A;
  const BlockVector& b;
  const std::vector<std::unique_ptr<ProxOperator>>& prox;
  DataMap* data;
  OpCache* shared_cache;  // Solver::set_shared_cache (null: none)
  BlockVector& u;
  std::vector<BlockVector>&x, &y, &y_prev;
};
struct TwoBlockParts {
  int num_constraints;
  const AffineOperator& constr_H;
  const std::vector<std::unique_ptr<ProxOperator>>& prox;
  DataMap* data;
  BlockVector &x, &z, &u, &z_prev;
};

// The route of the problem, or null: the lasso structure, then the ZERO-term structure
// (multi-block driver); the lasso structure in two-block form.
std::unique_ptr<FusedRoute> RecogniseMultiBlockRoute(const MultiBlockParts& parts);
std::unique_ptr<FusedRoute> RecogniseTwoBlockRoute(const TwoBlockParts& parts);

}  // namespace eps
