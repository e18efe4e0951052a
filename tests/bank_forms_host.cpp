// Stand-alone host program over csrc/tuner_plan.hpp, csrc/upconv_plan.hpp and csrc/polyfir_plan.hpp:
// prints the form the plan headers give for the shapes on its command line, one line per shape, so
// tests/test_bank_sweep_cpu.py can hold the form classes of tests/test_bank_sweep_cases.py against the
// code that dispatches the kernels.  Built with AddressSanitizer and UBSan and run as a child process.
//
//   bank_forms_host tuner D L [D L ...]      ->  tuner D L staged NF R
//   bank_forms_host upconv I L [I L ...]     ->  upconv I L NF FA A
//   bank_forms_host polyfir L D K [...]      ->  polyfir L D K Lp Dp T
//   bank_forms_host tuner-all                ->  every (staged, NF, R) that form() returns over
//                                                D = 1..2048 and a ladder of tap counts
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>

#include "polyfir_plan.hpp"
#include "tuner_plan.hpp"
#include "upconv_plan.hpp"

static unsigned long arg(const char* s) { return std::strtoul(s, nullptr, 10); }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* fam = argv[1];
    if (!std::strcmp(fam, "tuner-all")) {
        std::set<std::tuple<int, unsigned, unsigned>> seen;
        for (uint32_t D = 1; D <= sdrgpu::tuner::kMaxDecim; ++D)
            for (unsigned long L : {1ul, 2ul, 7ul, 64ul, 333ul, 1024ul, 2049ul, 4096ul}) {
                const sdrgpu::tuner::Form f = sdrgpu::tuner::form(D, L);
                seen.insert({f.staged ? 1 : 0, f.NF, f.R});
            }
        for (const auto& t : seen) std::printf("tuner-all %d %u %u\n", std::get<0>(t), std::get<1>(t), std::get<2>(t));
        return 0;
    }
    const int per = !std::strcmp(fam, "polyfir") ? 3 : 2;
    if ((argc - 2) % per) return 2;
    for (int i = 2; i + per <= argc; i += per) {
        const unsigned long a = arg(argv[i]), b = arg(argv[i + 1]);
        if (!std::strcmp(fam, "tuner")) {
            const sdrgpu::tuner::Form f = sdrgpu::tuner::form((uint32_t)a, b);
            std::printf("tuner %lu %lu %d %u %u\n", a, b, f.staged ? 1 : 0, f.NF, f.R);
        } else if (!std::strcmp(fam, "upconv")) {
            const sdrgpu::upconv::Form f = sdrgpu::upconv::form((uint32_t)a, b);
            std::printf("upconv %lu %lu %u %u %u\n", a, b, f.NF, f.FA, f.A);
        } else if (!std::strcmp(fam, "polyfir")) {
            const unsigned long k = arg(argv[i + 2]);
            const sdrgpu::polyfir::Geometry g = sdrgpu::polyfir::geometry((uint32_t)a, (uint32_t)b, k);
            std::printf("polyfir %lu %lu %lu %u %u %u\n", a, b, k, g.Lp, g.Dp, g.T);
        } else {
            return 2;
        }
    }
    return 0;
}
