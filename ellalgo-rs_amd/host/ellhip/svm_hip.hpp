// svm_hip.hpp -- `SvmOracle` (src/oracles/svm_oracle.rs:4-58) backed by the device-side oracle of
// include/ellhip_svm.h, plus the device-resident form of the driver loop it is used with.  Same constructor
// arguments, method name and return shape as the reference, so it plugs into the generic driver of
// cutting_plane.hpp (`cutting_plane_optim(omega, space, gamma, options)`) exactly like the reference's struct
// plugs into src/cutting_plane.rs; `cutting_plane_optim_device` runs the same loop without the centre, the
// gradient or the cut value ever leaving HBM.
#pragma once

#include <cstdint>
#include <optional>
#include <utility>
#include <vector>

#include "../../../include/ellhip_svm.h"
#include "ell_hip.hpp"

namespace ellhip {

class SvmOracleHip {
  public:
    using CutChoice = SingleCut;             // type CutChoice = SingleCut (:22)
    using Cut = std::pair<Arr, SingleCut>;

    // SvmOracle::new(data, labels) (:11-19): `data` is the m x nfeat table, row-major
    SvmOracleHip(const Arr& data, std::size_t nfeat, const std::vector<int32_t>& labels, int device = -1)
        : m_(labels.size()), nfeat_(nfeat) {
        if (nfeat == 0 || data.size() != m_ * nfeat) throw Error(ELLHIP_E_INVALID, "data must be m x nfeat");
        check(ellhip_svm_create(&h_, (int64_t)m_, (int64_t)nfeat, data.data(), labels.data(), device),
              "ellhip_svm_create");
    }
    SvmOracleHip(const SvmOracleHip&) = delete;
    SvmOracleHip& operator=(const SvmOracleHip&) = delete;
    SvmOracleHip(SvmOracleHip&& o) noexcept : h_(o.h_), m_(o.m_), nfeat_(o.nfeat_) { o.h_ = nullptr; }
    ~SvmOracleHip() { ellhip_svm_destroy(h_); }

    // impl OracleOptim<Arr> (:21-58); shrunk is always true
    std::pair<Cut, bool> assess_optim(const Arr& x, double& gamma) {
        if (x.size() != nfeat_ + 1) throw Error(ELLHIP_E_INVALID, "assess_optim: dimension mismatch");
        Arr g(nfeat_ + 1);
        double beta = 0.0;
        int shrunk = 0;
        check(ellhip_svm_assess_optim(h_, x.data(), &gamma, g.data(), &beta, &shrunk), "ellhip_svm_assess_optim");
        return {Cut{std::move(g), SingleCut{beta}}, shrunk != 0};
    }
    std::size_t ndim() const { return nfeat_ + 1; }
    ellhip_svm* handle() { return h_; }

  private:
    ellhip_svm* h_ = nullptr;
    std::size_t m_ = 0, nfeat_ = 0;
};

// cutting_plane_optim (src/cutting_plane.rs:286-313) with both sides on the device.
template <int VARIANT>
std::pair<std::optional<Arr>, std::size_t> cutting_plane_optim_device(SvmOracleHip& omega, SpaceHip<VARIANT>& space,
                                                                      double& gamma, const Options& options) {
    Arr x_best(space.ndim());
    int has_best = 0;
    int64_t niter = 0;
    check(ellhip_svm_optim(space.handle(), omega.handle(), &gamma, (int64_t)options.max_iters, options.tolerance,
                           x_best.data(), &has_best, &niter),
          "ellhip_svm_optim");
    if (!has_best) return {std::nullopt, (std::size_t)niter};
    return {std::move(x_best), (std::size_t)niter};
}

}  // namespace ellhip
