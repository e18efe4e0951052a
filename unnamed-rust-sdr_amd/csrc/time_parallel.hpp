// time_parallel.hpp -- "speculative segments": a serial recurrence made time-parallel, once
// for the PLL (pll.hip) and the biquad (biquad.hip).  DESIGN.md 3.5/3.6 have the measurements.
//
// A recurrence that forgets its initial state -- a PLL that is tracking, a stable biquad -- comes
// to agree BIT FOR BIT with the true trajectory some time after any start on the same input
// (configs[3]'s FM channels: the whole PLL state after a median 3.4 k, max 12 k samples; a biquad
// within a few pole time constants).  So each channel's block is cut into segments that run at
// once, one lane each:
//  * tp_segment (pass 1).  A segment runs `warm` samples of warm-up from the policy's warm-up
//    start state (no outputs), records the state it reached at its start (the guess), then
//    produces its outputs, recording a checkpoint every ck samples, and its end state.  A segment
//    whose warm-up reaches back to the block start runs from the carried state: its guess is true.
//  * tp_rerun (parallel re-run of the segments whose warm-up missed).  A segment's true start
//    state is its predecessor's end state, and pass 1's end state of the predecessor IS that
//    state whenever the predecessor ended on the true trajectory (its guess was right, or its
//    trajectory met the true one before its end -- the common case).  So every segment whose
//    guess differs from pass 1's end of its predecessor is re-run from that end state, until it
//    meets its own pass-1 trajectory at a checkpoint (rstop = +intervals run) or to its end
//    (rstop = -intervals, end state in end2).
//  * tp_walk (one lane per channel) walks the segments in order with the TRUE state (segment 0
//    started from the carried state).  Where a segment's guess equals the true state bit for bit
//    and nothing overwrote it, its outputs are the serial ones (same state, same inputs, same
//    arithmetic) and its end state is true; so is a re-run's that started from the true state.
//    Any other segment -- the warm-up missed and the re-run started from a wrong state, or such
//    a re-run overwrote outputs of a segment whose guess was right -- is computed again from the
//    true state, up to the first checkpoint its trajectory meets (from there on the stored
//    outputs are exact) and at least over the overwritten intervals.
// Every output is therefore the serial recurrence's; only the time depends on how many segments
// miss (none, typically; all of them for a chaotic, unlocked loop, which then costs one serial
// pass more than the serial kernel).
//
// The bodies are templates over a recurrence policy P, built per channel by the calling kernel:
//     P::State, P::kWords             the state, a struct of 32-bit words, and how many of its
//                                     leading words two trajectories must share to have met
//     P::warm_from(t0, warm) -> tw    where the warm-up of the segment starting at t0 begins;
//                                     0 = at the block start, from the carried state
//     p.load() / p.store(s)           the channel's carried state
//     p.warm_state(tw)                the state a warm-up starts from at sample tw > 0
//     p.template run<STORE>(s, a, b)  samples [a, b) through the recurrence; STORE: outputs too
//     p.miss()                        count one segment whose guess missed
// Plain C++ with no HIP in it, so the scheme also runs on the host (tests/time_parallel_host.cpp);
// whatever is device-only comes in through the policy.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define SDRGPU_TP_FN __device__ __forceinline__
#else
#define SDRGPU_TP_FN
#endif

namespace sdrgpu {

// Plan and scratch of one time-parallel block: ceil(n / seg) = nseg >= 2 segments per channel,
// `warm` samples of warm-up, a checkpoint every ck samples (ck divides seg).  States are indexed
// g = segment * nch + channel.
template <class State>
struct TpSpec {
    long seg = 0, warm = 0, ck = 0, nseg = 0;
    State* guess = nullptr;  // [nseg][nch] the state each warm-up reached at its segment's start
    State* end = nullptr;    // [nseg][nch] pass 1's state at the segment's end
    State* end2 = nullptr;   // [nseg][nch] a re-run's end state, where it ran to the end
    State* ckpt = nullptr;   // [nseg][nch][seg / ck - 1] pass 1's states at t0 + (j + 1) ck
    // per segment: +k = the re-run met pass 1's trajectory after k intervals, -k = it ran k
    // intervals (to the end) without meeting it, 0 = not re-run
    int* rstop = nullptr;
    unsigned long long* recomputed = nullptr;  // segments whose guess missed (zeroed per block)
};

template <int WORDS, class State>
SDRGPU_TP_FN bool tp_same(const State& a, const State& b) {
    static_assert(WORDS * sizeof(unsigned) <= sizeof(State), "more words than the state has");
    bool eq = true;
    for (int i = 0; i < WORDS; ++i) {
        unsigned x, y;
        __builtin_memcpy(&x, reinterpret_cast<const char*>(&a) + i * sizeof(unsigned), sizeof(unsigned));
        __builtin_memcpy(&y, reinterpret_cast<const char*>(&b) + i * sizeof(unsigned), sizeof(unsigned));
        eq &= x == y;
    }
    return eq;
}

// checkpoint interval j of the segment [t0, t1): samples [a, b); false past the (ragged) end
template <class State>
SDRGPU_TP_FN bool tp_interval(const TpSpec<State>& sp, long t0, long t1, long j, long& a, long& b) {
    a = t0 + j * sp.ck;
    b = j + 1 < sp.seg / sp.ck && a + sp.ck < t1 ? a + sp.ck : t1;
    return a < b;
}

template <class P>
SDRGPU_TP_FN void tp_segment(const P& p, const TpSpec<typename P::State>& sp, long nch, long n,
                             long ch, long sg) {
    using State = typename P::State;
    const long g = sg * nch + ch, t0 = sg * sp.seg, t1 = t0 + sp.seg < n ? t0 + sp.seg : n;
    const long tw = P::warm_from(t0, sp.warm);
    State s = tw == 0 ? p.load() : p.warm_state(tw);
    p.template run<false>(s, tw, t0);
    sp.guess[g] = s;
    const long nck = sp.seg / sp.ck;
    State* cp = sp.ckpt + g * (nck - 1);
    long a, b;
    for (long j = 0; j < nck && tp_interval(sp, t0, t1, j, a, b); ++j) {
        p.template run<true>(s, a, b);
        if (j + 1 < nck) cp[j] = s;
    }
    sp.end[g] = s;
}

// segments sg >= 1 (segment 0 starts from the carried state)
template <class P>
SDRGPU_TP_FN void tp_rerun(const P& p, const TpSpec<typename P::State>& sp, long nch, long n,
                           long ch, long sg) {
    using State = typename P::State;
    const long g = sg * nch + ch, t0 = sg * sp.seg, t1 = t0 + sp.seg < n ? t0 + sp.seg : n;
    if (P::warm_from(t0, sp.warm) == 0 || tp_same<P::kWords>(sp.guess[g], sp.end[g - nch])) {
        sp.rstop[g] = 0;
        return;
    }
    State t = sp.end[g - nch];
    const long nck = sp.seg / sp.ck;
    const State* cp = sp.ckpt + g * (nck - 1);
    int k = 0;
    bool met = false;
    long a, b;
    for (long j = 0; j < nck && !met && tp_interval(sp, t0, t1, j, a, b); ++j) {
        p.template run<true>(t, a, b);
        ++k;
        met = j + 1 < nck && tp_same<P::kWords>(cp[j], t);
    }
    sp.rstop[g] = met ? k : -k;
    if (!met) sp.end2[g] = t;
}

template <class P>
SDRGPU_TP_FN void tp_walk(const P& p, const TpSpec<typename P::State>& sp, long nch, long n,
                          long ch) {
    using State = typename P::State;
    State t = sp.end[ch];  // segment 0 started from the carried state: exact
    for (long sg = 1; sg < sp.nseg; ++sg) {
        const long g = sg * nch + ch, t0 = sg * sp.seg, t1 = t0 + sp.seg < n ? t0 + sp.seg : n;
        const bool hit = P::warm_from(t0, sp.warm) == 0 || tp_same<P::kWords>(sp.guess[g], t);
        const int rs = sp.rstop[g];
        if (hit && rs == 0) {  // pass 1 ran from the true state and nothing overwrote it
            t = sp.end[g];
            continue;
        }
        if (!hit) {
            p.miss();
            if (rs != 0 && tp_same<P::kWords>(sp.end[g - nch], t)) {  // re-run from the true state: exact
                t = rs > 0 ? sp.end[g] : sp.end2[g];
                continue;
            }
        }
        const long nck = sp.seg / sp.ck, over = rs < 0 ? -rs : rs;
        const State* cp = sp.ckpt + g * (nck - 1);
        bool met = false;
        long a, b;
        for (long j = 0; j < nck && !(met && j >= over) && tp_interval(sp, t0, t1, j, a, b); ++j) {
            p.template run<true>(t, a, b);
            met = j + 1 < nck && tp_same<P::kWords>(cp[j], t);
        }
        if (met) t = sp.end[g];
    }
    p.store(t);
}

// ---- host side: the checkpoint choice, the scratch layout, the check before a launch ----

// checkpoints every ck samples: at most 16 per segment, ck a multiple of 8 dividing seg and no
// shorter than min_ck
inline long tp_checkpoint_interval(long seg, long min_ck) {
    for (long d = 16; d >= 2; --d)
        if (seg % (8 * d) == 0 && seg / d >= min_ck) return seg / d;
    return seg;
}

// Scratch of a block whose seg, ck and nseg are set: guess, end, end2, the checkpoints, a 64-byte
// block for the counter, then the re-run marks.
template <class State>
size_t tp_scratch_bytes(const TpSpec<State>& sp, long nch) {
    const size_t nstate = (size_t)sp.nseg * (size_t)nch;
    return (size_t)(2 + sp.seg / sp.ck) * nstate * sizeof(State) + 64 + nstate * sizeof(int);
}
template <class State>
void tp_lay_out(TpSpec<State>& sp, long nch, void* scratch) {
    static_assert(sizeof(State) % sizeof(unsigned long long) == 0, "the counter follows the states");
    const size_t nstate = (size_t)sp.nseg * (size_t)nch, nck = (size_t)(sp.seg / sp.ck - 1);
    sp.guess = static_cast<State*>(scratch);
    sp.end = sp.guess + nstate;
    sp.end2 = sp.end + nstate;
    sp.ckpt = nck ? sp.end2 + nstate : nullptr;
    sp.recomputed = reinterpret_cast<unsigned long long*>(sp.end2 + (1 + nck) * nstate);
    sp.rstop = reinterpret_cast<int*>(sp.recomputed + 8);
}

// What the kernels rely on for a block of n samples whose loads and stores move `chunk` samples
template <class State>
bool tp_spec_valid(const TpSpec<State>& sp, long n, long chunk) {
    return sp.seg > 0 && sp.seg % chunk == 0 && sp.ck > 0 && sp.ck % chunk == 0 && sp.seg % sp.ck == 0 &&
           sp.nseg == (n + sp.seg - 1) / sp.seg && sp.nseg >= 2 && sp.guess && sp.end && sp.end2 &&
           sp.rstop && sp.recomputed && (sp.seg / sp.ck == 1 || sp.ckpt);
}

}  // namespace sdrgpu
