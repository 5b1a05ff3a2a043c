// lmi_loop_hip.hpp -- the round-robin oracle of tests/lmi_tests.rs:142-171, generalised to J blocks, over the device-side
// LMI oracles of lmi_hip.hpp, in two forms with the same results to the bit:
//   RoundRobinLmiHost   the walk on the host, one ellhip_lmi_assess_feas per station; plugs into the generic drivers of
//                       cutting_plane.hpp like the reference's `MyOracle` plugs into src/cutting_plane.rs
//   LmiLoopHip          the problem handle of include/ellhip_lmi_loop.h: the walk on the device, `optim` / `feas` run the
//                       driver loops without the centre, the gradient or the cut value ever leaving HBM
// Both borrow the blocks (LMIOracleHip / LMI0OracleHip handles): the caller keeps them alive.
#pragma once

#include <cstdint>
#include <optional>
#include <utility>
#include <vector>

#include "../../../include/ellhip_lmi_loop.h"
#include "lmi_hip.hpp"

namespace ellhip {

class RoundRobinLmiHost {
  public:
    using CutChoice = SingleCut;
    using Cut = std::pair<Arr, SingleCut>;

    RoundRobinLmiHost(std::vector<ellhip_lmi*> blocks, std::size_t n, std::optional<Arr> c = std::nullopt)
        : blocks_(std::move(blocks)), n_(n), c_(std::move(c)) {}

    // impl OracleOptim<Arr>
    std::pair<Cut, bool> assess_optim(const Arr& xc, double& gamma) {
        const int J = (int)blocks_.size();
        double f0 = 0.0;
        for (std::size_t k = 0; k < n_; ++k) f0 = f0 + (*c_)[k] * xc[k];
        for (int step = 0; step < J + 1; ++step) {
            idx_ = idx_ >= J ? 0 : idx_ + 1;
            if (idx_ < J) {
                if (auto cut = block(idx_, xc)) return {std::move(*cut), false};
            } else {
                const double fj = f0 - gamma;
                if (fj > 0.0) return {Cut{*c_, SingleCut{fj}}, false};
                gamma = f0;
            }
        }
        return {Cut{*c_, SingleCut{0.0}}, true};
    }
    // impl OracleFeas<Arr>
    std::optional<Cut> assess_feas(const Arr& xc) {
        const int J = (int)blocks_.size();
        for (int step = 0; step < J; ++step) {
            idx_ = idx_ >= J - 1 ? 0 : idx_ + 1;
            if (auto cut = block(idx_, xc)) return cut;
        }
        return std::nullopt;
    }
    int idx() const { return idx_; }
    std::size_t block_calls() const { return block_calls_; }  // ellhip_lmi_assess_feas calls made so far

  private:
    std::optional<Cut> block(int j, const Arr& xc) {
        block_calls_ += 1;
        Arr g(n_, 0.0);
        double ep = 0.0;
        if (check(ellhip_lmi_assess_feas(blocks_[(std::size_t)j], xc.data(), g.data(), &ep), "ellhip_lmi_assess_feas") == 0)
            return std::nullopt;
        return Cut{std::move(g), SingleCut{ep}};
    }
    std::vector<ellhip_lmi*> blocks_;
    std::size_t n_;
    std::optional<Arr> c_;
    int idx_ = -1;
    std::size_t block_calls_ = 0;
};

class LmiLoopHip {
  public:
    LmiLoopHip(const std::vector<ellhip_lmi*>& blocks, std::size_t n, const std::optional<Arr>& c = std::nullopt) : n_(n) {
        if (c && c->size() != n) throw Error(ELLHIP_E_INVALID, "c must have n entries");
        check(ellhip_lmi_loop_create(&h_, blocks.data(), (int64_t)blocks.size(), c ? c->data() : nullptr),
              "ellhip_lmi_loop_create");
    }
    LmiLoopHip(const LmiLoopHip&) = delete;
    LmiLoopHip& operator=(const LmiLoopHip&) = delete;
    LmiLoopHip(LmiLoopHip&& o) noexcept : h_(o.h_), n_(o.n_) { o.h_ = nullptr; }
    ~LmiLoopHip() { ellhip_lmi_loop_destroy(h_); }

    int idx() const {
        int v = 0;
        check(ellhip_lmi_loop_get_idx(h_, &v), "ellhip_lmi_loop_get_idx");
        return v;
    }
    void set_idx(int v) { check(ellhip_lmi_loop_set_idx(h_, v), "ellhip_lmi_loop_set_idx"); }

    // cutting_plane_optim (src/cutting_plane.rs:286-313) with both sides on the device
    template <int VARIANT>
    std::pair<std::optional<Arr>, std::size_t> optim(SpaceHip<VARIANT>& space, double& gamma, const Options& options) {
        Arr x_best(n_);
        int has_best = 0;
        int64_t niter = 0;
        check(ellhip_lmi_loop_optim(space.handle(), h_, &gamma, (int64_t)options.max_iters, options.tolerance,
                                    x_best.data(), &has_best, &niter),
              "ellhip_lmi_loop_optim");
        if (!has_best) return {std::nullopt, (std::size_t)niter};
        return {std::move(x_best), (std::size_t)niter};
    }
    // cutting_plane_feas (src/cutting_plane.rs:205-227)
    template <int VARIANT>
    std::pair<std::optional<Arr>, std::size_t> feas(SpaceHip<VARIANT>& space, const Options& options) {
        Arr x(n_);
        int ok = 0;
        int64_t niter = 0;
        check(ellhip_lmi_loop_feas(space.handle(), h_, (int64_t)options.max_iters, options.tolerance, x.data(), &ok, &niter),
              "ellhip_lmi_loop_feas");
        if (!ok) return {std::nullopt, (std::size_t)niter};
        return {std::move(x), (std::size_t)niter};
    }
    ellhip_lmi_loop* handle() { return h_; }

  private:
    ellhip_lmi_loop* h_ = nullptr;
    std::size_t n_ = 0;
};

}  // namespace ellhip
