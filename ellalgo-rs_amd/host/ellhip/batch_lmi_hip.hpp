// batch_lmi_hip.hpp -- B independent LMI-constrained problems solved side by side on the device
// (include/ellhip_batch_lmi.h): the C++ counterpart of
//     for b in 0..B { cutting_plane_optim(&mut omega[b], &mut space[b], &mut gamma[b], &options) }
// with omega[b] the round-robin oracle of tests/lmi_tests.rs:142-171 over J LMIOracle / LMI0Oracle blocks and space[b]
// the b-th ellipsoid of an EllBatchHip.  Bit-identical to the CPU arithmetic.
// BatchLmiHip::streamed and ::streamed_shared (include/ellhip_batch_lmi_streamed.h) take n up to 1024 and solve on an
// EllBatchStreamedHip or an EllStableBatchStreamedHip.
#pragma once

#include <cstdint>
#include <optional>
#include <vector>

#include "../../../include/ellhip_batch_lmi_streamed.h"
#include "../../../include/ellhip_batch_stable_loops.h"
#include "ell_batch_hip.hpp"

namespace ellhip {

// one problem: mat_f[j] is [n][m_j][m_j] row-major, mat_b[j] is [m_j][m_j] (empty mat_b: LMI0 form), c is [n] (empty c:
// feasibility problem)
struct LmiProblem {
    std::vector<Arr> mat_f;
    std::vector<Arr> mat_b;
    Arr c;
};

struct BatchLmiResult {
    std::vector<std::optional<Arr>> x_best;  // (feas: the feasible point)
    std::vector<std::size_t> niter;
    std::vector<CutStatus> status;
};

class BatchLmiHip {
  public:
    // m[j]: the size of block j; every problem has the same n, J and m
    BatchLmiHip(const std::vector<LmiProblem>& problems, std::size_t n, const std::vector<std::size_t>& m, int device = -1)
        : BatchLmiHip(problems, n, m, device, false, false) {}
    // the same problems for n up to 1024: optim / feas then take an EllBatchStreamedHip or an EllStableBatchStreamedHip
    static BatchLmiHip streamed(const std::vector<LmiProblem>& problems, std::size_t n, const std::vector<std::size_t>& m,
                                int device = -1) {
        return BatchLmiHip(problems, n, m, device, true, false);
    }
    // one pencil for every problem: mat_f is taken from problems[0], mat_b and c from each problem
    static BatchLmiHip streamed_shared(const std::vector<LmiProblem>& problems, std::size_t n,
                                       const std::vector<std::size_t>& m, int device = -1) {
        return BatchLmiHip(problems, n, m, device, true, true);
    }
    BatchLmiHip(const BatchLmiHip&) = delete;
    BatchLmiHip& operator=(const BatchLmiHip&) = delete;
    BatchLmiHip(BatchLmiHip&& o) noexcept : h_(o.h_), B_(o.B_), n_(o.n_), J_(o.J_) { o.h_ = nullptr; }
    ~BatchLmiHip() { ellhip_batch_lmi_destroy(h_); }

    std::size_t size() const { return B_; }
    std::size_t ndim() const { return n_; }
    std::size_t blocks() const { return J_; }

    // cutting_plane_optim (src/cutting_plane.rs:286-313) for every problem; gamma has B entries and is updated
    // (spaces: an EllBatchHip, an EllStableBatchHip through include/ellhip_batch_stable_loops.h, or an EllBatchStreamedHip
    // or an EllStableBatchStreamedHip through include/ellhip_batch_lmi_streamed.h)
    template <int VARIANT, bool STREAMED>
    BatchLmiResult optim(BatchHip<VARIANT, STREAMED>& spaces, Arr& gamma, const Options& options) {
        if (gamma.size() != B_) throw Error(ELLHIP_E_INVALID, "gamma must have B entries");
        Arr x(B_ * n_);
        std::vector<int32_t> has(B_), status(B_);
        std::vector<int64_t> niter(B_);
        const auto entry = loop_entry(spaces, "ellhip_batch_lmi_optim", ellhip_batch_lmi_optim, ellhip_batch_lmi_optim_stable,
                                      ellhip_batch_lmi_optim_streamed, ellhip_batch_lmi_optim_streamed_stable);
        check(entry.fn(spaces.handle(), h_, gamma.data(), (int64_t)options.max_iters, options.tolerance, x.data(), has.data(),
                    niter.data(), status.data()),
              entry.name.c_str());
        return result(x, has, niter, status);
    }
    // cutting_plane_feas (:205-227) for every problem
    template <int VARIANT, bool STREAMED>
    BatchLmiResult feas(BatchHip<VARIANT, STREAMED>& spaces, const Options& options) {
        Arr x(B_ * n_);
        std::vector<int32_t> has(B_), status(B_);
        std::vector<int64_t> niter(B_);
        const auto entry = loop_entry(spaces, "ellhip_batch_lmi_feas", ellhip_batch_lmi_feas, ellhip_batch_lmi_feas_stable,
                                      ellhip_batch_lmi_feas_streamed, ellhip_batch_lmi_feas_streamed_stable);
        check(entry.fn(spaces.handle(), h_, (int64_t)options.max_iters, options.tolerance, x.data(), has.data(), niter.data(),
                    status.data()),
              entry.name.c_str());
        return result(x, has, niter, status);
    }
    std::vector<int32_t> idx() const {
        std::vector<int32_t> v(B_);
        check(ellhip_batch_lmi_get_idx(h_, v.data()), "ellhip_batch_lmi_get_idx");
        return v;
    }
    void reset_idx() { check(ellhip_batch_lmi_set_idx(h_, nullptr), "ellhip_batch_lmi_set_idx"); }
    void set_chunk(std::size_t iters) { check(ellhip_batch_lmi_set_chunk(h_, (int64_t)iters), "ellhip_batch_lmi_set_chunk"); }
    ellhip_batch_lmi* handle() { return h_; }

  private:
    BatchLmiHip(const std::vector<LmiProblem>& problems, std::size_t n, const std::vector<std::size_t>& m, int device,
                bool streamed, bool shared)
        : B_(problems.size()), n_(n), J_(m.size()) {
        if (problems.empty()) throw Error(ELLHIP_E_INVALID, "need at least one problem");
        const bool has_b = !problems[0].mat_b.empty(), has_c = !problems[0].c.empty();
        Arr f, bm, c;
        std::vector<int64_t> m64(m.begin(), m.end());
        for (std::size_t j = 0; j < J_; ++j) {
            bool first = true;
            for (const LmiProblem& p : problems) {
                if (p.mat_f.size() != J_ || p.mat_f[j].size() != n * m[j] * m[j] || (has_b && p.mat_b.size() != J_) ||
                    (has_b && p.mat_b[j].size() != m[j] * m[j]) || (!has_b && !p.mat_b.empty()))
                    throw Error(ELLHIP_E_INVALID, "every problem needs the same shape");
                if (!shared || first) f.insert(f.end(), p.mat_f[j].begin(), p.mat_f[j].end());
                if (has_b) bm.insert(bm.end(), p.mat_b[j].begin(), p.mat_b[j].end());
                first = false;
            }
        }
        if (has_c)
            for (const LmiProblem& p : problems) {
                if (p.c.size() != n) throw Error(ELLHIP_E_INVALID, "c must have n entries");
                c.insert(c.end(), p.c.begin(), p.c.end());
            }
        if (streamed)
            check(ellhip_batch_lmi_create_streamed(&h_, (int64_t)B_, (int64_t)n_, (int64_t)J_, m64.data(), f.data(),
                                                   shared ? 1 : 0, has_b ? bm.data() : nullptr, has_c ? c.data() : nullptr,
                                                   device),
                  "ellhip_batch_lmi_create_streamed");
        else
            check(ellhip_batch_lmi_create(&h_, (int64_t)B_, (int64_t)n_, (int64_t)J_, m64.data(), f.data(),
                                          has_b ? bm.data() : nullptr, has_c ? c.data() : nullptr, device),
                  "ellhip_batch_lmi_create");
    }
    BatchLmiResult result(const Arr& x, const std::vector<int32_t>& has, const std::vector<int64_t>& niter,
                          const std::vector<int32_t>& status) const {
        BatchLmiResult r;
        for (std::size_t b = 0; b < B_; ++b) {
            if (has[b]) r.x_best.emplace_back(Arr(x.begin() + b * n_, x.begin() + (b + 1) * n_));
            else r.x_best.emplace_back(std::nullopt);
            r.niter.push_back((std::size_t)niter[b]);
            r.status.push_back(static_cast<CutStatus>(status[b]));
        }
        return r;
    }

    ellhip_batch_lmi* h_ = nullptr;
    std::size_t B_ = 0, n_ = 0, J_ = 0;
};

}  // namespace ellhip
