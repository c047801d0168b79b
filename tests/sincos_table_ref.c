/* Host side of tests/test_sincos_table_host.py: the remainder table of the 20-bit Box-Muller angle (klara.jl_amd/csrc/detmath.h), filled by the
 * routine the kernels fill it with (kd_sincos_rem_entry) and read back through kd_sincos_rotate, against the arithmetic form — TEST INFRASTRUCTURE.
 * Compiled at test time: gcc -O2 -std=gnu11 -ffp-contract=off. */
#include <stdint.h>
#include <string.h>
#include "detmath.h"

void st_fill(double* T)                                  /* T[2m] = sin y, T[2m + 1] = cos y - 1 of remainder m */
{
    for (uint32_t m = 0; m < KD_SCREM_ENTRIES; ++m) kd_sincos_rem_entry(m, &T[2 * m], &T[2 * m + 1]);
}

static int same(double a, double b) { return kd_d2u(a) == kd_d2u(b); }

/* every angle index k < 2^20: table form against kd_sincos2pi_bits(kd_angle_bits20(k << 12)); returns the number of angles at which a bit
 * differs (first_bad: the first of them or -1).  sy_all / dc_all receive kd_sincos_rem of every angle's own bits (the values a table replaces);
 * low12 != 0 fills the 12 bits of the word below the angle with a pattern: they belong to the radius and must not matter. */
int64_t st_compare(const double* T, int low12, double* sy_all, double* dc_all, int64_t* first_bad)
{
    int64_t bad = 0;
    *first_bad = -1;
    for (uint32_t k = 0; k < (1u << 20); ++k) {
        const uint32_t wb = (k << 12) | (low12 ? (k * 2654435761u) >> 20 : 0u);
        const uint64_t bits = kd_angle_bits20(wb);
        double s0, c0, s1, c1;
        kd_sincos2pi_bits(bits, &s0, &c0);
        const uint32_t kk = wb >> 12, m = kk & (KD_SCREM_ENTRIES - 1u), j = kk >> 12;
        kd_sincos_rotate(j, T[2 * m], T[2 * m + 1], &s1, &c1);
        if (!same(s0, s1) || !same(c0, c1)) { if (bad == 0) *first_bad = (int64_t)k; ++bad; }
        kd_sincos_rem(bits, &sy_all[k], &dc_all[k]);
    }
    return bad;
}

/* the double-argument form at u = (k + 1/2) 2^-20 (what the selftest's ops 2 / 3 evaluate): the same bits as the 20-bit angle */
int64_t st_compare_double_form(const double* T)
{
    int64_t bad = 0;
    for (uint32_t k = 0; k < (1u << 20); ++k) {
        double s0, c0, s1, c1;
        kd_sincos2pi(((double)k + 0.5) * 0x1p-20, &s0, &c0);
        kd_sincos_rotate(k >> 12, T[2 * (k & 4095u)], T[2 * (k & 4095u) + 1], &s1, &c1);
        bad += !same(s0, s1) || !same(c0, c1);
    }
    return bad;
}
