// batch_maxcut_hip.hpp -- B independent max-cut problems of one size solved side by side on the device
// (include/ellhip_batch_maxcut.h): the C++ counterpart of
//     for b in 0..B { cutting_plane_optim(&mut omega[b], &mut space[b], &mut gamma[b], &options) }
// with omega[b] a MaxcutOracle (src/oracles/maxcut_oracle.rs:4-50) over its own or a shared weight table, and space[b] the
// b-th ellipsoid of an EllBatchHip, an EllStableBatchHip (n <= 128), an EllBatchStreamedHip or an EllStableBatchStreamedHip
// (n <= 1024) of dimension n.  Bit-identical to the CPU arithmetic.
#pragma once

#include <cstdint>
#include <optional>
#include <utility>
#include <vector>

#include "../../../include/ellhip_batch_maxcut.h"
#include "ell_batch_hip.hpp"

namespace ellhip {

struct BatchMaxcutResult {
    std::vector<std::optional<Arr>> x_best;
    std::vector<std::size_t> niter;
    std::vector<CutStatus> status;
};

class BatchMaxcutHip {
  public:
    // ((Arr, SingleCut), bool) (:21) and the cut value the reference keeps in a local
    struct Cut {
        Arr grad;
        double beta;
        bool shrunk;
        double cut_value;
    };

    // weights: row-major n x n when `shared` (one table for every problem), else B x n x n
    BatchMaxcutHip(std::size_t B, std::size_t n, const Arr& weights, bool shared, int device = -1) : B_(B), n_(n) {
        if (weights.size() != (shared ? 1 : B) * n * n) throw Error(ELLHIP_E_INVALID, "weights must be [B] x n x n");
        check(ellhip_batch_maxcut_create(&h_, (int64_t)B, (int64_t)n, weights.data(), shared ? 1 : 0, device),
              "ellhip_batch_maxcut_create");
    }
    BatchMaxcutHip(const BatchMaxcutHip&) = delete;
    BatchMaxcutHip& operator=(const BatchMaxcutHip&) = delete;
    BatchMaxcutHip(BatchMaxcutHip&& o) noexcept : h_(o.h_), B_(o.B_), n_(o.n_) { o.h_ = nullptr; }
    ~BatchMaxcutHip() { ellhip_batch_maxcut_destroy(h_); }

    std::size_t size() const { return B_; }
    std::size_t ndim() const { return n_; }

    // omega[b].assess_optim(&x[b], &mut gamma[b]) for every b (:21-49)
    std::vector<Cut> assess_optim(const std::vector<Arr>& x, Arr& gamma) {
        if (x.size() != B_ || gamma.size() != B_) throw Error(ELLHIP_E_INVALID, "x and gamma must have B entries");
        Arr flat;
        for (const Arr& row : x) {
            if (row.size() != n_) throw Error(ELLHIP_E_INVALID, "dimension mismatch");
            flat.insert(flat.end(), row.begin(), row.end());
        }
        Arr g(B_ * n_), beta(B_), cut(B_);
        std::vector<int32_t> shrunk(B_);
        check(ellhip_batch_maxcut_assess_optim(h_, flat.data(), gamma.data(), g.data(), beta.data(), shrunk.data(), cut.data()),
              "ellhip_batch_maxcut_assess_optim");
        std::vector<Cut> r;
        for (std::size_t b = 0; b < B_; ++b)
            r.push_back(Cut{Arr(g.begin() + b * n_, g.begin() + (b + 1) * n_), beta[b], shrunk[b] != 0, cut[b]});
        return r;
    }
    // cutting_plane_optim (src/cutting_plane.rs:286-313) for every problem; gamma has B entries and is updated
    template <int VARIANT, bool STREAMED>
    BatchMaxcutResult optim(BatchHip<VARIANT, STREAMED>& spaces, Arr& gamma, const Options& options) {
        if (gamma.size() != B_) throw Error(ELLHIP_E_INVALID, "gamma must have B entries");
        Arr x(B_ * n_);
        std::vector<int32_t> has(B_), status(B_);
        std::vector<int64_t> niter(B_);
        const auto entry = loop_entry(spaces, "ellhip_batch_maxcut_optim", ellhip_batch_maxcut_optim,
                                      ellhip_batch_maxcut_optim_stable, ellhip_batch_maxcut_optim_streamed,
                                      ellhip_batch_maxcut_optim_streamed_stable);
        check(entry.fn(spaces.handle(), h_, gamma.data(), (int64_t)options.max_iters, options.tolerance, x.data(), has.data(),
                    niter.data(), status.data()),
              entry.name.c_str());
        BatchMaxcutResult r;
        for (std::size_t b = 0; b < B_; ++b) {
            if (has[b]) r.x_best.emplace_back(Arr(x.begin() + b * n_, x.begin() + (b + 1) * n_));
            else r.x_best.emplace_back(std::nullopt);
            r.niter.push_back((std::size_t)niter[b]);
            r.status.push_back(static_cast<CutStatus>(status[b]));
        }
        return r;
    }
    void set_chunk(std::size_t iters) {
        check(ellhip_batch_maxcut_set_chunk(h_, (int64_t)iters), "ellhip_batch_maxcut_set_chunk");
    }
    ellhip_batch_maxcut* handle() { return h_; }

  private:
    ellhip_batch_maxcut* h_ = nullptr;
    std::size_t B_ = 0, n_ = 0;
};

}  // namespace ellhip
