// The scalar side of the ICP iteration loop (libwave_amd/csrc/wm_icp_ctl.hpp), on the host and away from any device: the
// step record's bit layout (what every solve kernel packs and the loop unpacks) and the certificate policy (which search
// kernel an iteration gets, decided from the record of iteration it - lag).  The expectations are the rules as the loop
// stated them before they were moved into that header -- written out here independently, not read off it.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "wm_icp_ctl.hpp"

static int bad = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            ++bad;                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
        }                                                               \
    } while (0)

static float top16(float v) {  // a float truncated to its top 16 bits (bfloat16 by truncation)
    unsigned u;
    std::memcpy(&u, &v, 4);
    u &= 0xFFFF0000u;
    std::memcpy(&v, &u, 4);
    return v;
}
static float frac16(float f) {  // clamped to [0, 1], rounded to 1 / 65535
    const float c = f < 0.f ? 0.f : (f > 1.f ? 1.f : f);
    return (float) (unsigned) (c * 65535.f + 0.5f) / 65535.f;
}

static void record_round_trip() {
    const int iters[] = {1, 2, 65535, 65536 + 3};
    const float disps[] = {0.f, 1e-3f, 0.15f, 3e38f};
    const float fracs[] = {0.f, 1.f / 65535.f, 0.05f, 0.4f, 1.f, -0.1f, 1.7f};
    for (int it : iters)
        for (float d : disps)
            for (float fc : fracs)
                for (float fu : fracs) {
                    const unsigned long long w = wm::pack_step_record(it, d, fc, fu);
                    const wm::StepRecord r = wm::unpack_step_record(w);
                    CHECK(r.iter == ((unsigned) it & 0xFFFFu));
                    CHECK(r.disp == top16(d));
                    CHECK(r.changed == frac16(fc));
                    CHECK(r.unsettled == frac16(fu));
                    CHECK(wm::record_is_for(w, (unsigned) it));
                    CHECK(!wm::record_is_for(w, (unsigned) it + 1u));
                    CHECK(!wm::record_is_for(w, (unsigned) it - 1u));
                    // the layout itself: [iteration : 16 | bfloat16 : 16 | changed : 16 | searched : 16]
                    CHECK((w >> 48) == ((unsigned long long) it & 0xFFFFull));
                    CHECK((w & 0xFFFFull) == (unsigned long long) (frac16(fu) * 65535.f + 0.5f));
                }
    const unsigned needs[] = {0u, 1u, 2u, 65535u, 65536u, 65536u + 3u, 131072u};
    for (unsigned need : needs) CHECK(!wm::record_is_for(0ull, need));  // "not written yet", whatever is waited for
    const int its[] = {0, 1, 7, 65535, 65536 + 3, 1 << 24};
    for (int it : its) {
        const unsigned long long w = wm::pack_done_word(1, it);
        CHECK(wm::done_word_done(w) && wm::done_word_iterations(w) == (unsigned) it);
        CHECK((w & 1ull) == 1ull && (w >> 1) == (unsigned long long) it);
        CHECK(wm::pack_done_word(0, it) == 0ull);
        CHECK(!wm::done_word_done(wm::pack_done_word(0, it)));
    }
}

// ---- the policy, with the defaults: cert_changed 0.05, cert_unsettled 0.40, lag 2
constexpr float kThr = 0.03f;  // cert_disp x the level-0 cell
constexpr int kLag = 2, kMaxIt = 64;
static wm::CertPolicy policy(int cert_from = -1) {
    return wm::CertPolicy(cert_from >= -1, cert_from, kThr, 0.05f, 0.40f, kLag, kMaxIt);
}
static wm::StepRecord rec(float disp, float changed, float unsettled) { return wm::StepRecord{0u, disp, changed, unsettled}; }
// one launched iteration, as the loop drives the policy: decide, then tell it what ran
static bool step(wm::CertPolicy &P, int it, const wm::StepRecord *seen) {
    const bool on = P.decide(it, it >= kLag ? seen : nullptr);
    if (on) P.ran_cert(it);
    else P.ran_full(it);
    return on;
}

static void policy_rules() {
    const wm::StepRecord moving = rec(2.f * kThr, 0.01f, 0.f), churning = rec(0.5f * kThr, 0.05f, 0.f),
                         settled = rec(0.5f * kThr, 0.01f, 0.f);
    {  // 1: off while the step is large or many matches change; also at the very thresholds (strict comparisons)
        wm::CertPolicy P = policy();
        const wm::StepRecord at_thr = rec(kThr, 0.01f, 0.f);
        for (int it = 0; it < 12; ++it) CHECK(!step(P, it, it % 3 == 0 ? &moving : (it % 3 == 1 ? &churning : &at_thr)));
        CHECK(!P.bounds_valid);
    }
    {  // 2, 3, 11: on at the first record with both below, first certificate iteration kind 2, later ones kind 1
        wm::CertPolicy P = policy();
        for (int it = 0; it < 5; ++it) {
            CHECK(!P.decide(it, it >= kLag ? &moving : nullptr));
            CHECK(!P.ran_full(it) && !P.bounds_valid);
        }
        CHECK(P.decide(5, &settled));
        CHECK(!P.ran_cert(5));  // no bounds to go by: the launch's argument is false ...
        CHECK(P.kind[5] == 2 && P.bounds_valid);
        CHECK(P.decide(6, &settled));
        CHECK(P.ran_cert(6));  // ... and true from the second on
        CHECK(P.kind[6] == 1 && P.bounds_valid);
        // 4: iteration 7 sees iteration 5's record -- a first certificate launch searched everything, it says nothing
        const wm::StepRecord all_searched = rec(0.5f * kThr, 0.01f, 1.0f);
        CHECK(P.decide(7, &all_searched));
        CHECK(P.ran_cert(7) && P.kind[7] == 1);
        // 5: iteration 8 sees iteration 6's, a kind-1 record: a share at the limit stays, above it turns off
        const wm::StepRecord at_limit = rec(0.5f * kThr, 0.01f, 0.40f), above = rec(0.5f * kThr, 0.01f, 0.41f);
        wm::CertPolicy Q = P;
        CHECK(Q.decide(8, &at_limit));
        CHECK(!P.decide(8, &above));
        CHECK(P.ran_full(8));  // the bounds were valid before it
        CHECK(!P.bounds_valid && P.kind[8] == 0);
        // 2: not back on from the record of a certificate iteration (7: kind 1), whatever it says ...
        CHECK(!P.decide(9, &settled));
        P.ran_full(9);
        // ... but from the next record of a full search (8)
        CHECK(P.decide(10, &settled));
        CHECK(!P.ran_cert(10) && P.kind[10] == 2);
    }
    {  // 6: a step above 3 x the threshold turns it off, 3 x itself does not; a kind-2 record's step counts too
        wm::CertPolicy P = policy();
        for (int it = 0; it < 3; ++it) step(P, it, &settled);
        CHECK(P.cert_on && P.kind[2] == 2);
        const wm::StepRecord big = rec(3.5f * kThr, 0.01f, 0.f), edge = rec(top16(3.f * kThr), 0.01f, 0.f);
        CHECK(step(P, 3, &edge));
        CHECK(!P.decide(4, &big));  // (iteration 2's record: kind 2)
        wm::CertPolicy Q = policy();
        for (int it = 0; it < 4; ++it) step(Q, it, &settled);
        CHECK(Q.kind[3] == 1);
        CHECK(step(Q, 4, &settled));
        CHECK(!Q.decide(5, &big));  // (iteration 3's record: kind 1)
    }
    for (int k : {0, 1, 4, 9}) {  // 7: forced from iteration k on, whatever the records say
        wm::CertPolicy P = policy(k);
        const wm::StepRecord wild = rec(100.f * kThr, 1.f, 1.f);
        for (int it = 0; it < 14; ++it) CHECK(step(P, it, it & 1 ? &wild : &settled) == (it >= k));
        CHECK(P.kind[k] == 2 && P.kind[k + 1] == 1);
    }
    {  // 8: never (cert_from = -2: can_cert false)
        wm::CertPolicy P = policy(-2);
        for (int it = 0; it < 14; ++it) CHECK(!step(P, it, &settled));
        CHECK(!P.bounds_valid);
    }
    {  // 9, 10, 11: the resident kernel
        wm::CertPolicy P = policy();
        for (int it = 0; it < 3; ++it) step(P, it, &settled);  // on at 2 (kind 2), bounds valid
        CHECK(P.decide(3, &settled) && P.bounds_valid);
        CHECK(P.ran_resident(3, 5, 2));  // iterations 3 .. 7 inside, left by its policy: the loop goes on
        for (int k = 3; k < 8; ++k) CHECK(P.kind[k] == 1);
        CHECK(P.bounds_valid && !P.cert_on);
        for (int it = 8; it < 8 + kLag; ++it) {  // off for exactly kLag iterations, whatever the records say
            CHECK(!P.decide(it, &settled));
            P.ran_full(it);
        }
        CHECK(P.cert_hold == 0);
        wm::CertPolicy R = P;
        CHECK(!R.decide(10, &moving));  // from records again: iteration 8's, a full search's ...
        CHECK(P.decide(10, &settled));  // ... which turns it on when it is small enough
        CHECK(!P.ran_cert(10) && P.kind[10] == 2);
        wm::CertPolicy Q = policy();
        for (int it = 0; it < 3; ++it) step(Q, it, &moving);
        // a resident launch without valid bounds: its first iteration is kind 2
        Q.cert_on = true;
        CHECK(Q.ran_resident(3, 4, 4));
        CHECK(Q.kind[3] == 2 && Q.kind[4] == 1 && Q.kind[6] == 1 && Q.kind[7] == 0 && Q.bounds_valid && Q.cert_on);
        CHECK(Q.ran_resident(7, 0, 3) && Q.cert_hold == 0);  // a wait gave up, nothing ran: goes on, launched
        CHECK(!Q.ran_resident(7, 2, 1));                     // 10: done ends the loop
    }
}

int main() {
    record_round_trip();
    policy_rules();
    std::printf("failed checks: %d\n", bad);
    return bad != 0;
}
