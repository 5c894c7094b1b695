// Prints the nearest-first walk of wm_zigzag.hpp for tests/test_zigzag_cpu.py: one line per (lo, c, hi, frac):
//   lo c hi frac | the hi - lo + 1 coordinates in visiting order | zigzag_remaining at every step (hex floats)
#include <cstdio>

#include "wm_zigzag.hpp"

int main() {
    const float fracs[] = {0.f, 0.125f, 0.5f, 0.75f, 1.f};
    for (int lo = -2; lo <= 3; ++lo)
        for (int hi = lo; hi <= lo + 12; ++hi)
            for (int c = lo; c <= hi; ++c)
                for (float frac : fracs) {
                    std::printf("%d %d %d %a |", lo, c, hi, (double) frac);
                    for (int k = 0; k <= hi - lo; ++k) std::printf(" %d", wm::zigzag_coord(k, lo, c, hi));
                    std::printf(" |");
                    for (int k = 0; k <= hi - lo + 1; ++k) std::printf(" %a", (double) wm::zigzag_remaining(k, lo, c, hi, frac));
                    std::printf("\n");
                }
    return 0;
}
