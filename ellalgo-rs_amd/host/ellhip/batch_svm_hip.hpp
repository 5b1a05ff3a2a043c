// batch_svm_hip.hpp -- B independent SVM problems of one shape solved side by side on the device
// (include/ellhip_batch_svm.h): the C++ counterpart of
//     for b in 0..B { cutting_plane_optim(&mut omega[b], &mut space[b], &mut gamma[b], &options) }
// with omega[b] a SvmOracle (src/oracles/svm_oracle.rs:4-58) over its own labels and its own or a shared table, and
// space[b] the b-th ellipsoid of an EllBatchHip of dimension nfeat + 1.  Bit-identical to the CPU arithmetic.
// BatchSvmHip::streamed (include/ellhip_batch_svm_streamed.h) takes up to 1023 features and solves on an EllBatchStreamedHip
// or an EllStableBatchStreamedHip.
#pragma once

#include <cstdint>
#include <optional>
#include <utility>
#include <vector>

#include "../../../include/ellhip_batch_stable_loops.h"
#include "../../../include/ellhip_batch_svm_streamed.h"
#include "ell_batch_hip.hpp"

namespace ellhip {

struct BatchSvmResult {
    std::vector<std::optional<Arr>> x_best;
    std::vector<std::size_t> niter;
    std::vector<CutStatus> status;
};

class BatchSvmHip {
  public:
    using Cut = std::pair<Arr, double>;  // (Arr, f64) (:21)
    // what the last scan found: the reference's locals min_idx / min_val (:28-29)
    struct Last {
        std::size_t min_idx;
        double min_val;
    };

    // data: row-major m x nfeat when `shared` (one table for every problem), else B x m x nfeat; labels: B x m
    BatchSvmHip(std::size_t B, std::size_t m, std::size_t nfeat, const Arr& data, bool shared,
                const std::vector<int32_t>& labels, int device = -1)
        : BatchSvmHip(B, m, nfeat, data, shared, labels, device, false) {}
    // the same problems for nfeat up to 1023: optim then takes an EllBatchStreamedHip or an EllStableBatchStreamedHip
    static BatchSvmHip streamed(std::size_t B, std::size_t m, std::size_t nfeat, const Arr& data, bool shared,
                                const std::vector<int32_t>& labels, int device = -1) {
        return BatchSvmHip(B, m, nfeat, data, shared, labels, device, true);
    }
    BatchSvmHip(const BatchSvmHip&) = delete;
    BatchSvmHip& operator=(const BatchSvmHip&) = delete;
    BatchSvmHip(BatchSvmHip&& o) noexcept : h_(o.h_), B_(o.B_), m_(o.m_), n_(o.n_) { o.h_ = nullptr; }
    ~BatchSvmHip() { ellhip_batch_svm_destroy(h_); }

    std::size_t size() const { return B_; }
    std::size_t samples() const { return m_; }
    std::size_t ndim() const { return n_; }

    // the m margins of every problem at x[b]
    std::vector<Arr> margins(const std::vector<Arr>& x) {
        const Arr flat = flatten(x);
        Arr mg(B_ * m_);
        check(ellhip_batch_svm_margins(h_, flat.data(), mg.data()), "ellhip_batch_svm_margins");
        std::vector<Arr> r;
        for (std::size_t b = 0; b < B_; ++b) r.emplace_back(mg.begin() + b * m_, mg.begin() + (b + 1) * m_);
        return r;
    }
    // omega[b].assess_optim(&x[b], &mut gamma[b]) for every b (:27-57); `shrunk` is always true
    std::vector<Cut> assess_optim(const std::vector<Arr>& x, Arr& gamma) {
        const Arr flat = flatten(x);
        Arr g(B_ * n_), beta(B_);
        gamma.assign(B_, 0.0);
        check(ellhip_batch_svm_assess_optim(h_, flat.data(), gamma.data(), g.data(), beta.data()),
              "ellhip_batch_svm_assess_optim");
        std::vector<Cut> r;
        for (std::size_t b = 0; b < B_; ++b) r.emplace_back(Arr(g.begin() + b * n_, g.begin() + (b + 1) * n_), beta[b]);
        return r;
    }
    std::vector<Last> last() const {
        std::vector<int64_t> idx(B_);
        Arr val(B_);
        check(ellhip_batch_svm_last(h_, idx.data(), val.data()), "ellhip_batch_svm_last");
        std::vector<Last> r;
        for (std::size_t b = 0; b < B_; ++b) r.push_back(Last{(std::size_t)idx[b], val[b]});
        return r;
    }
    // cutting_plane_optim (src/cutting_plane.rs:286-313) for every problem; gamma has B entries and is updated
    // (spaces: an EllBatchHip, an EllStableBatchHip through include/ellhip_batch_stable_loops.h, or an EllBatchStreamedHip
    // or an EllStableBatchStreamedHip through include/ellhip_batch_svm_streamed.h)
    template <int VARIANT, bool STREAMED>
    BatchSvmResult optim(BatchHip<VARIANT, STREAMED>& spaces, Arr& gamma, const Options& options) {
        if (gamma.size() != B_) throw Error(ELLHIP_E_INVALID, "gamma must have B entries");
        Arr x(B_ * n_);
        std::vector<int32_t> has(B_), status(B_);
        std::vector<int64_t> niter(B_);
        const auto entry = loop_entry(spaces, "ellhip_batch_svm_optim", ellhip_batch_svm_optim, ellhip_batch_svm_optim_stable,
                                      ellhip_batch_svm_optim_streamed, ellhip_batch_svm_optim_streamed_stable);
        check(entry.fn(spaces.handle(), h_, gamma.data(), (int64_t)options.max_iters, options.tolerance, x.data(), has.data(),
                    niter.data(), status.data()),
              entry.name.c_str());
        BatchSvmResult r;
        for (std::size_t b = 0; b < B_; ++b) {
            if (has[b]) r.x_best.emplace_back(Arr(x.begin() + b * n_, x.begin() + (b + 1) * n_));
            else r.x_best.emplace_back(std::nullopt);
            r.niter.push_back((std::size_t)niter[b]);
            r.status.push_back(static_cast<CutStatus>(status[b]));
        }
        return r;
    }
    void set_chunk(std::size_t iters) { check(ellhip_batch_svm_set_chunk(h_, (int64_t)iters), "ellhip_batch_svm_set_chunk"); }
    ellhip_batch_svm* handle() { return h_; }

  private:
    BatchSvmHip(std::size_t B, std::size_t m, std::size_t nfeat, const Arr& data, bool shared,
                const std::vector<int32_t>& labels, int device, bool streamed)
        : B_(B), m_(m), n_(nfeat + 1) {
        if (data.size() != (shared ? 1 : B) * m * nfeat) throw Error(ELLHIP_E_INVALID, "data must be [B] x m x nfeat");
        if (labels.size() != B * m) throw Error(ELLHIP_E_INVALID, "labels must be B x m");
        check((streamed ? ellhip_batch_svm_create_streamed : ellhip_batch_svm_create)(
                  &h_, (int64_t)B, (int64_t)m, (int64_t)nfeat, data.data(), shared ? 1 : 0, labels.data(), device),
              streamed ? "ellhip_batch_svm_create_streamed" : "ellhip_batch_svm_create");
    }
    Arr flatten(const std::vector<Arr>& x) const {
        if (x.size() != B_) throw Error(ELLHIP_E_INVALID, "x must have B rows");
        Arr flat;
        for (const Arr& row : x) {
            if (row.size() != n_) throw Error(ELLHIP_E_INVALID, "dimension mismatch");
            flat.insert(flat.end(), row.begin(), row.end());
        }
        return flat;
    }

    ellhip_batch_svm* h_ = nullptr;
    std::size_t B_ = 0, m_ = 0, n_ = 0;
};

}  // namespace ellhip
