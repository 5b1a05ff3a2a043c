// batch_lowpass_hip.hpp -- B independent low-pass filter design problems of one filter length solved side by side on
// the device (include/ellhip_batch_lowpass.h): the C++ counterpart of
//     for b in 0..B { cutting_plane_optim(&mut omega[b], &mut space[b], &mut gamma[b], &options) }
// with omega[b] a LowpassOracle (src/oracles/lowpass_oracle.rs:7-151) of its own band edges and ripple limits and
// space[b] the b-th ellipsoid of an EllBatchHip.  Bit-identical to the CPU arithmetic.  BatchLowpassHip::streamed
// (include/ellhip_batch_lowpass_streamed.h) takes filter lengths up to 1024 and solves on an EllBatchStreamedHip or, through
// include/ellhip_batch_lowpass_streamed_stable.h, on an EllStableBatchStreamedHip.
#pragma once

#include <cstdint>
#include <optional>
#include <utility>
#include <vector>

#include "../../../include/ellhip_batch_lowpass_streamed_stable.h"
#include "../../../include/ellhip_batch_stable_loops.h"
#include "ell_batch_hip.hpp"

namespace ellhip {

// LowpassOracle::new's arguments after ndim (:23)
struct LowpassSpec {
    double wpass, wstop, lp_sq, up_sq, sp_sq;
};

struct BatchLowpassResult {
    std::vector<std::optional<Arr>> x_best;  // (feas: the feasible point)
    std::vector<std::size_t> niter;
    std::vector<CutStatus> status;
};

class BatchLowpassHip {
  public:
    using Cut = std::pair<Arr, ParallelCut>;  // pub type Cut = (Arr, ParallelCut) (:5)
    // the structs' public fields (:8-20), read back from the device
    struct Fields {
        bool more_alt;
        int idx1, idx2, idx3, kmax, nwpass, nwstop;
        double fmax, sp_sq;
    };

    // spectrum: empty = computed as the reference does; else the shared table, row-major 15 ndim x ndim
    BatchLowpassHip(std::size_t ndim, const std::vector<LowpassSpec>& specs, const Arr& spectrum = Arr(), int device = -1)
        : BatchLowpassHip(ndim, specs, spectrum, device, false) {}
    // the same problems for ndim up to 1024: optim / feas then take an EllBatchStreamedHip or an EllStableBatchStreamedHip
    static BatchLowpassHip streamed(std::size_t ndim, const std::vector<LowpassSpec>& specs, const Arr& spectrum = Arr(),
                                    int device = -1) {
        return BatchLowpassHip(ndim, specs, spectrum, device, true);
    }
    BatchLowpassHip(const BatchLowpassHip&) = delete;
    BatchLowpassHip& operator=(const BatchLowpassHip&) = delete;
    BatchLowpassHip(BatchLowpassHip&& o) noexcept : h_(o.h_), B_(o.B_), n_(o.n_) { o.h_ = nullptr; }
    ~BatchLowpassHip() { ellhip_batch_lowpass_destroy(h_); }

    std::size_t size() const { return B_; }
    std::size_t ndim() const { return n_; }

    // omega[b].assess_feas(&x[b]) for every b (:58-133)
    std::vector<std::optional<Cut>> assess_feas(const std::vector<Arr>& x) {
        const Arr flat = flatten(x);
        Arr g(B_ * n_), b0(B_), b1(B_);
        std::vector<int32_t> hb1(B_), cut(B_);
        check(ellhip_batch_lowpass_assess_feas(h_, flat.data(), g.data(), b0.data(), hb1.data(), b1.data(), cut.data()),
              "ellhip_batch_lowpass_assess_feas");
        std::vector<std::optional<Cut>> r;
        for (std::size_t b = 0; b < B_; ++b) {
            if (cut[b]) r.emplace_back(make_cut(g, b0, hb1, b1, b));
            else r.emplace_back(std::nullopt);
        }
        return r;
    }
    // omega[b].assess_optim(&x[b], &mut gamma[b]) for every b (:139-150); nullopt where the reference would panic
    std::vector<std::optional<std::pair<Cut, bool>>> assess_optim(const std::vector<Arr>& x, Arr& gamma) {
        if (gamma.size() != B_) throw Error(ELLHIP_E_INVALID, "gamma must have B entries");
        const Arr flat = flatten(x);
        Arr g(B_ * n_), b0(B_), b1(B_);
        std::vector<int32_t> hb1(B_), shrunk(B_), rc(B_);
        check(ellhip_batch_lowpass_assess_optim(h_, flat.data(), gamma.data(), g.data(), b0.data(), hb1.data(), b1.data(),
                                                shrunk.data(), rc.data()),
              "ellhip_batch_lowpass_assess_optim");
        std::vector<std::optional<std::pair<Cut, bool>>> r;
        for (std::size_t b = 0; b < B_; ++b) {
            if (rc[b] == 1) r.emplace_back(std::make_pair(make_cut(g, b0, hb1, b1, b), shrunk[b] != 0));
            else r.emplace_back(std::nullopt);
        }
        return r;
    }
    // cutting_plane_optim (src/cutting_plane.rs:286-313) for every problem; gamma has B entries and is updated
    // (spaces: an EllBatchHip, an EllStableBatchHip through include/ellhip_batch_stable_loops.h, an EllBatchStreamedHip
    // through include/ellhip_batch_lowpass_streamed.h, or an EllStableBatchStreamedHip through
    // include/ellhip_batch_lowpass_streamed_stable.h)
    template <int VARIANT, bool STREAMED>
    BatchLowpassResult optim(BatchHip<VARIANT, STREAMED>& spaces, Arr& gamma, const Options& options) {
        if (gamma.size() != B_) throw Error(ELLHIP_E_INVALID, "gamma must have B entries");
        Arr x(B_ * n_);
        std::vector<int32_t> has(B_), status(B_);
        std::vector<int64_t> niter(B_);
        const auto entry = loop_entry(spaces, "ellhip_batch_lowpass_optim", ellhip_batch_lowpass_optim,
                                      ellhip_batch_lowpass_optim_stable, ellhip_batch_lowpass_optim_streamed,
                                      ellhip_batch_lowpass_optim_streamed_stable);
        check(entry.fn(spaces.handle(), h_, gamma.data(), (int64_t)options.max_iters, options.tolerance, x.data(), has.data(),
                    niter.data(), status.data()),
              entry.name.c_str());
        return result(x, has, niter, status);
    }
    // cutting_plane_feas (:205-227) for every problem
    template <int VARIANT, bool STREAMED>
    BatchLowpassResult feas(BatchHip<VARIANT, STREAMED>& spaces, const Options& options) {
        Arr x(B_ * n_);
        std::vector<int32_t> has(B_), status(B_);
        std::vector<int64_t> niter(B_);
        const auto entry = loop_entry(spaces, "ellhip_batch_lowpass_feas", ellhip_batch_lowpass_feas,
                                      ellhip_batch_lowpass_feas_stable, ellhip_batch_lowpass_feas_streamed,
                                      ellhip_batch_lowpass_feas_streamed_stable);
        check(entry.fn(spaces.handle(), h_, (int64_t)options.max_iters, options.tolerance, x.data(), has.data(), niter.data(),
                    status.data()),
              entry.name.c_str());
        return result(x, has, niter, status);
    }
    std::vector<Fields> fields() const {
        std::vector<int32_t> i(7 * B_);
        Arr d(2 * B_);
        check(ellhip_batch_lowpass_state(h_, i.data(), d.data()), "ellhip_batch_lowpass_state");
        std::vector<Fields> r;
        for (std::size_t b = 0; b < B_; ++b) {
            const int32_t* p = i.data() + 7 * b;
            r.push_back(Fields{p[0] != 0, p[1], p[2], p[3], p[4], p[5], p[6], d[2 * b], d[2 * b + 1]});
        }
        return r;
    }
    Arr spectrum() const {
        Arr s(15 * n_ * n_);
        check(ellhip_batch_lowpass_get_spectrum(h_, s.data()), "ellhip_batch_lowpass_get_spectrum");
        return s;
    }
    void reset() { check(ellhip_batch_lowpass_reset(h_), "ellhip_batch_lowpass_reset"); }
    void set_chunk(std::size_t iters) { check(ellhip_batch_lowpass_set_chunk(h_, (int64_t)iters), "ellhip_batch_lowpass_set_chunk"); }
    ellhip_batch_lowpass* handle() { return h_; }

  private:
    BatchLowpassHip(std::size_t ndim, const std::vector<LowpassSpec>& specs, const Arr& spectrum, int device, bool streamed)
        : B_(specs.size()), n_(ndim) {
        if (specs.empty()) throw Error(ELLHIP_E_INVALID, "need at least one problem");
        if (!spectrum.empty() && spectrum.size() != 15 * ndim * ndim) throw Error(ELLHIP_E_INVALID, "spectrum must be 15n x n");
        Arr wp, ws, lp, up, sp;
        for (const LowpassSpec& s : specs) {
            wp.push_back(s.wpass);
            ws.push_back(s.wstop);
            lp.push_back(s.lp_sq);
            up.push_back(s.up_sq);
            sp.push_back(s.sp_sq);
        }
        check((streamed ? ellhip_batch_lowpass_create_streamed : ellhip_batch_lowpass_create)(
                  &h_, (int64_t)B_, (int64_t)n_, wp.data(), ws.data(), lp.data(), up.data(), sp.data(),
                  spectrum.empty() ? nullptr : spectrum.data(), device),
              streamed ? "ellhip_batch_lowpass_create_streamed" : "ellhip_batch_lowpass_create");
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
    Cut make_cut(const Arr& g, const Arr& b0, const std::vector<int32_t>& hb1, const Arr& b1, std::size_t b) const {
        return Cut{Arr(g.begin() + b * n_, g.begin() + (b + 1) * n_),
                   ParallelCut{b0[b], hb1[b] ? std::optional<double>(b1[b]) : std::nullopt}};
    }
    BatchLowpassResult result(const Arr& x, const std::vector<int32_t>& has, const std::vector<int64_t>& niter,
                              const std::vector<int32_t>& status) const {
        BatchLowpassResult r;
        for (std::size_t b = 0; b < B_; ++b) {
            if (has[b]) r.x_best.emplace_back(Arr(x.begin() + b * n_, x.begin() + (b + 1) * n_));
            else r.x_best.emplace_back(std::nullopt);
            r.niter.push_back((std::size_t)niter[b]);
            r.status.push_back(static_cast<CutStatus>(status[b]));
        }
        return r;
    }

    ellhip_batch_lowpass* h_ = nullptr;
    std::size_t B_ = 0, n_ = 0;
};

}  // namespace ellhip
