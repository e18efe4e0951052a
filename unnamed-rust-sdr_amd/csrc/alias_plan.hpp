// alias_plan.hpp -- what a device-pointer call of a serial recurrence (sdrgpu_pll_process_dev,
// sdrgpu_biquad_process_dev) does when its output rows overlap its input rows, free of HIP: the
// handles (abi_pll.cpp, abi_biquad.cpp) and a stand-alone host test (tests/alias_plan_host.cpp)
// share it.
//
// The serial kernels (biquad_kernel; pll_kernel and pll_split_kernel) run one row per lane: a
// lane loads 8 samples of its row (the PLL one chunk further ahead), steps them and stores the 8
// results, then the ragged tail sample by sample.  Nothing orders one lane against another, and
// a lane's own stores reach memory before its later loads.  So an overlapped call is right in
// place only if no store can land on an input byte that is still to be read:
//   - the output and input rows have one pitch in bytes (with one row the pitch plays no part),
//   - an output element is no larger than an input element,
//   - the output rows start at or before the input rows, delta = in - out >= 0 bytes, so sample
//     j's result, at out + j*out_elem, ends at or before in + (j + 1)*in_elem: a lane's stores
//     never pass its own loads,
//   - and with several rows delta <= pitch - n*in_elem: row r's results, which start delta
//     bytes before its inputs, stay clear of row r - 1's last sample; they end before row r's
//     own inputs do, so they cannot reach row r + 1 either.
// Exact in-place calls (delta 0, equal elements and leading dimensions) and the PLL's f32 rows
// written over its own c64 rows (ld_out = 2 ld_in) pass; f32 outputs over c64 inputs with one
// leading dimension, any forward shift and any row that reaches into another do not.  Every
// other overlap is answered by copy_input: the handle filters a device copy of the input span
// with its normal plan, time-parallel segments included.
//
// serial_in_place relies on a chunk's loads being issued before that chunk's stores, which the
// kernels' source order gives and their __restrict__ qualifiers do not take away while a chunk's
// results depend on its loads; test_biquad_in_place_long_block and test_pll_in_place_long_block
// pin it on the device.
#pragma once

#include <cstddef>
#include <cstdint>

namespace sdrgpu {
namespace alias {

enum class Plan {
    disjoint = 0,         // no byte of the two spans is shared: any plan may run
    serial_in_place = 1,  // overlapped, and the serial pass is right in place
    copy_input = 2,       // overlapped otherwise: run the normal plan on a copy of the input
};

// Rows of n elements (elem bytes each), row r at base + r*ld*elem.
struct Rows {
    uintptr_t base;
    size_t ld, n, elem;
};

// Bytes from the first row's start to the last row's end.
inline size_t span_bytes(size_t nrows, const Rows& r) {
    return nrows && r.n ? ((nrows - 1) * r.ld + r.n) * r.elem : 0;
}

inline bool spans_overlap(size_t nrows, const Rows& a, const Rows& b) {
    const size_t na = span_bytes(nrows, a), nb = span_bytes(nrows, b);
    return na && nb && a.base < b.base + nb && b.base < a.base + na;
}

inline Plan classify(size_t nrows, const Rows& in, const Rows& out) {
    if (!spans_overlap(nrows, in, out)) return Plan::disjoint;
    const size_t pitch = in.ld * in.elem;
    if (nrows > 1 && out.ld * out.elem != pitch) return Plan::copy_input;
    if (out.elem > in.elem || in.base < out.base) return Plan::copy_input;
    if (nrows > 1 && (in.ld < in.n || in.base - out.base > pitch - in.n * in.elem)) return Plan::copy_input;
    return Plan::serial_in_place;
}

// A call with two output row sets (the PLL's outputs and lock flags) takes the stronger answer.
inline Plan stronger(Plan a, Plan b) { return a > b ? a : b; }

}  // namespace alias
}  // namespace sdrgpu
