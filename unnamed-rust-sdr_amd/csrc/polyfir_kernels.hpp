// polyfir_kernels.hpp -- launch interface of the rational-rate polyphase FIR kernels (polyfir.hip).
#pragma once

#include <vector>

#include "common.hpp"
#include "polyfir_plan.hpp"

namespace sdrgpu {

// Which form a handle's shape takes (decided once, from L, D and ntaps alone, so rows, calls and
// partitions never change it).  staged: the tile's input span and its outputs fit the LDS budget
// with at least 64 super-frames per tile, and Lp <= 32.
struct PolyfirForm {
    bool staged = false;
    int NA = 0;    // super-frames per tile: 1024, 512, 256 (R = 4), 128 (R = 2) or 64 (R = 1)
    int R = 0;     // same-phase outputs per lane
    int Tpad = 0;  // row pitch of the phase image
    size_t lds_bytes = 0;
};
PolyfirForm polyfir_form(const polyfir::Geometry& g);

// The device tables of the staged form: image[i*Tpad + t] = h[p_i + L*t] (zero past the phase's
// last tap, never read), tab[i] = {qoff_i, taps of phase p_i}.
void polyfir_tables(const polyfir::Geometry& g, const PolyfirForm& f, const float* h, size_t ntaps,
                    std::vector<float>& image, std::vector<int2>& tab);

struct PolyfirArgs {
    const void* in = nullptr;   // rows of n_in samples, ld_in apart
    long ld_in = 0, n_in = 0;
    const void* hist = nullptr;  // rows of HL = T-1 samples: the inputs before in[0]
    void* hist_next = nullptr;   // the same after this call
    void* out = nullptr;         // rows of n_out samples, ld_out apart
    long ld_out = 0, n_out = 0;
    int rows = 0;
    bool cplx = false;           // C64 samples (else F32)
    const float* taps = nullptr;   // h[0..K)
    const float* image = nullptr;  // staged form
    const int2* tab = nullptr;
    int K = 0;
    polyfir::Geometry g;
    polyfir::Origin o;
};

// Enqueues the call's outputs (n_out > 0) and the history carry (n_in > 0) on s.
int polyfir_launch(const PolyfirForm& f, const PolyfirArgs& a, hipStream_t s);

}  // namespace sdrgpu
