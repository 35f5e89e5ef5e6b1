// drop_host.h -- the host side that the handles of the four gene-dropping sweeps (simu.hip, ident.hip, retain.hip, link.hip) share on
// top of sweep_device.h: the panels of a sweep in pairs of words, the timer of a panel's two phases, the body of genphi_*_levels and a
// result's way to the host.  Host functions only, no kernels; every including file gets its own copy (anonymous namespace).
#pragma once
#include "drop_plan.h"
#include "sweep_device.h"

namespace {

// The panels of a sweep over S simulations whose panel rows hold Pn pairs of words (128 columns): simu, ident, retain.  (link.hip counts
// its panels in simulations.)
struct DropPanels {
    int64_t total = 0;                       // the pairs of words of all S simulations
    int32_t pairs = 0, lanes_per_row = 0;    // pairs of a panel row
    int64_t n_panels = 0;
    void set(int64_t S, int64_t Pn)
    {
        total = (S + 127) / 128;
        pairs = static_cast<int32_t>(Pn);
        lanes_per_row = ::lanes_per_row(static_cast<int>(Pn));
        n_panels = (total + Pn - 1) / Pn;
    }
};

// The two timed phases of a panel: three events, created at the first begin() and destroyed on every path.  Work launched between
// end() and add() runs before add() returns but is in neither phase.
struct PhaseTimer {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    PhaseTimer() = default;
    PhaseTimer(const PhaseTimer &) = delete;
    PhaseTimer &operator=(const PhaseTimer &) = delete;
    ~PhaseTimer()
    {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int record(int k, hipStream_t stream)
    {
        GENPHI_HIP_TRY(hipEventRecord(e[k], stream));
        return GENPHI_OK;
    }
    int begin(hipStream_t stream)
    {
        for (hipEvent_t &x : e)
            if (!x) GENPHI_HIP_TRY(hipEventCreate(&x));
        return record(0, stream);
    }
    int middle(hipStream_t stream) { return record(1, stream); }
    int end(hipStream_t stream) { return record(2, stream); }
    // waits for end(); first += begin .. middle, second += middle .. end, in ms
    int add(double &first, double &second)
    {
        GENPHI_HIP_TRY(hipEventSynchronize(e[2]));
        float a = 0.f, b = 0.f;
        GENPHI_HIP_TRY(hipEventElapsedTime(&a, e[0], e[1]));
        GENPHI_HIP_TRY(hipEventElapsedTime(&b, e[1], e[2]));
        first += a;
        second += b;
        return GENPHI_OK;
    }
};

// The body of genphi_*_levels (h->plan is a DropRows); fn: the entry point's name.
template <typename H>
int drop_levels(const H *h, const char *fn, int64_t *n_live, int32_t *levels, int64_t *rows_per_level)
{
    if (!h) return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": NULL handle");
    const genphi::DropRows &pl = h->plan;
    put(n_live, pl.n_live);
    put(levels, pl.n_levels);
    if (rows_per_level)
        for (int k = 0; k < pl.n_levels; ++k) rows_per_level[k] = pl.level_rows[k];
    return GENPHI_OK;
}

// The body of a genphi_*_to_host for the result block h->*buf; fn: the entry point's name, who: "gen.simuIdentity", ..
template <typename H, typename T>
int result_to_host(H *h, void *out, DevBuf<T> H::*buf, const char *fn, const char *who)
{
    if (!h || !h->computed) return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": nothing computed");
    if (!out) return genphi_set_error(GENPHI_ERR_ARG, std::string(fn) + ": out is NULL");
    return h->copy_out(out, (h->*buf).get(), (h->*buf).bytes(), who);
}

}  // namespace
