// wm_icp_ctl.hpp -- the scalar side of the ICP iteration loop (icp_run_loop, wm_icp.hip): the record every solve
// publishes for the host that runs ahead of it, and the policy that picks an iteration's search kernel from those
// records.  No HIP types: the packers are compiled for the device (publish_step, wm_icp_step.hpp; k_late_solver,
// wm_nn_cert.hip), the readers and the policy for the host, and all of it by g++ away from any device
// (tests/cpp_host/icp_ctl_host.cpp).  This is the ONE place that knows the words' bit layout.
#pragma once
#include <math.h>

#include <vector>

#include "wm_math.hpp"

namespace wm {

// ---- iteration k's own record, pub[k]:
// [iteration : 16 | step size as bfloat16 : 16 | changed matches : 16 | searched by the certificate kernel : 16]
// -- fractions in 1 / 65535.  Never 0 for a published record's reader: an all-zero word is "not written yet".
struct StepRecord {
    unsigned iter;          // iterations finished when it was written, modulo 2^16
    float disp;             // the step's size (metres), truncated to its top 16 bits
    float changed;          // fraction of the handled queries whose match changed
    float unsettled;        // fraction the certificate kernel had to search (0 after a full search)
};

// (by reference: the device's callers hand in fields of a state held in LDS, and each is then read where it is used --
// by value the reads move ahead of the arithmetic and the solve kernels' code comes out in another order)
WM_HD unsigned long long pack_step_record(const int &iter, const float &step_disp, const float &frac_changed,
                                          const float &frac_unsettled) {
    const unsigned f_ch = (unsigned) (fminf(fmaxf(frac_changed, 0.f), 1.f) * 65535.f + 0.5f);
    const unsigned f_un = (unsigned) (fminf(fmaxf(frac_unsettled, 0.f), 1.f) * 65535.f + 0.5f);
    return ((unsigned long long) ((unsigned) iter & 0xFFFFu) << 48) |
           ((unsigned long long) (__builtin_bit_cast(unsigned, step_disp) >> 16) << 32) |
           ((unsigned long long) f_ch << 16) | (unsigned long long) f_un;
}

WM_HD StepRecord unpack_step_record(unsigned long long w) {
    StepRecord r;
    r.iter = (unsigned) (w >> 48);
    r.disp = __builtin_bit_cast(float, (unsigned) ((w >> 32) & 0xFFFFu) << 16);
    r.changed = (float) ((w >> 16) & 0xFFFFu) / 65535.f;
    r.unsettled = (float) (w & 0xFFFFu) / 65535.f;
    return r;
}

// is w the record written after `need` iterations?  (need = 65536 k has the iteration field 0: the word still is
// not the empty one unless everything else in it is zero too, and then the wait goes on to the done word)
WM_HD bool record_is_for(unsigned long long w, unsigned need) {
    return (unsigned) (w >> 48) == (need & 0xFFFFu) && w != 0ull;
}

// ---- the latest state, pub[0]: bit 0 = done, above it the number of iterations finished by then -- ONE word, so
// that a host that sees `done` before the last record knows whether that record is still to come.  0 while running.
WM_HD unsigned long long pack_done_word(int done, int iter) {
    return done ? (1ull | ((unsigned long long) (unsigned) iter << 1)) : 0ull;
}
WM_HD bool done_word_done(unsigned long long w) { return (w & 1ull) != 0ull; }
WM_HD unsigned done_word_iterations(unsigned long long w) { return (unsigned) (w >> 1); }

// ---- which search kernel iteration `it` gets: the full search (k_nn_grid) while the clouds still move, the
// certificate kernel (k_nn_cert) once a step is a small fraction of a grid cell.  Decided from the record of
// iteration it - lag alone, so the choice does not depend on when the host looks.  Host only.
// (The resident kernel leaves by a rule of its own -- k_late_solver, wm_nn_cert.hip -- on the unquantised values of the
// iteration it has just solved: not this function, and not to be merged with it.)
struct CertPolicy {
    bool can_cert;          // the certificate kernel may be used at all in this loop
    int cert_from;          // >= 0: forced, on from this iteration whatever the records say
    float cert_thr;         // on once a step moves the points by less than this (cert_disp x the level-0 cell) ...
    float cert_changed;     // ... AND fewer than this fraction of the matches changed in the last full search
    float cert_unsettled;   // off again when a certificate launch had to search more than this fraction
    int lag;                // the record seen before iteration `it` is iteration (it - lag)'s
    bool cert_on = false;
    bool bounds_valid = false;  // the previous search was a certificate launch: its per-query bounds still hold
    int cert_hold = 0;          // iterations for which the policy stays off after the resident kernel left by it
    std::vector<unsigned char> kind;  // which search iteration k got (0: full, 1: certificate, 2: its first launch)

    CertPolicy(bool can_cert_, int cert_from_, float cert_thr_, float cert_changed_, float cert_unsettled_, int lag_,
               int max_it)
        : can_cert(can_cert_), cert_from(cert_from_), cert_thr(cert_thr_), cert_changed(cert_changed_),
          cert_unsettled(cert_unsettled_), lag(lag_), kind((size_t) (max_it > 0 ? max_it : 0), 0) {}

    // certificate kernel for iteration `it`?  seen: the record of iteration it - lag (nullptr: none yet)
    bool decide(int it, const StepRecord *seen) {
        if (!can_cert) return cert_on;
        if (cert_hold > 0) {
            --cert_hold;
            cert_on = false;
        } else if (cert_from >= 0) {
            cert_on = it >= cert_from;
        } else if (seen && seen->disp >= 0.f) {
            // certify once a step is small AND few matches still change (on a scan whose density varies
            // by orders of magnitude the dense part keeps changing partners long after the step has
            // become small against the grid cell); back to full searches when a certificate launch had
            // to search a large share after all
            // (the record of a certificate launch that had no bounds to go by -- the first after full
            // searches -- says nothing: it searched everything)
            const unsigned char rec = (size_t) (it - lag) < kind.size() ? kind[(size_t) (it - lag)] : 0;
            if (!cert_on) {
                if (seen->disp < cert_thr && seen->changed < cert_changed && rec == 0) cert_on = true;
            } else if (rec == 1 && seen->unsettled > cert_unsettled) {
                cert_on = false;
            } else if (seen->disp > 3.f * cert_thr) {
                cert_on = false;
            }
        }
        return cert_on;
    }
    // what iteration `it` was given; both return whether the bounds were valid BEFORE it (the launch's argument)
    bool ran_full(int) {
        const bool had = bounds_valid;
        bounds_valid = false;
        return had;
    }
    bool ran_cert(int it) {
        const bool had = bounds_valid;
        if ((size_t) it < kind.size()) kind[(size_t) it] = had ? 1 : 2;
        bounds_valid = true;
        return had;
    }
    // the resident kernel ran `inside` iterations from `it` on and left for `reason` (1: done, 2: its policy,
    // 3: a wait gave up, 4: its budget); false: the registration is done
    bool ran_resident(int it, int inside, int reason) {
        for (int k = 0; k < inside && (size_t) (it + k) < kind.size(); ++k)
            kind[(size_t) (it + k)] = (k == 0 && !bounds_valid) ? 2 : 1;
        if (inside > 0) bounds_valid = true;
        if (reason == 2) {  // the policy: full searches again, and let the records catch up
            cert_on = false;
            cert_hold = lag;
        }
        return reason != 1;
    }
};

}  // namespace wm
