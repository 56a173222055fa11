// Stand-alone check of value_halvable / value_half_bits (tilespmv_amd/csrc/plan_tile_ops.h) over all 65,536 binary16 bit patterns, on the CPU.  Built and run by
// tests/test_value_half_cpu.py with AddressSanitizer and UBSan on the host side.  The half is decoded here by integer arithmetic of its own (no _Float16, no library call):
// sign, 5 exponent bits (bias 15), 10 mantissa bits.  Exit status 0 = everything holds; every failure is printed.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "plan_tile_ops.h"

static double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
static uint64_t to_bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

// the double with the value of half pattern h (finite patterns only), built from its fields
static double decode_half(unsigned h)
{
    const uint64_t sign = (uint64_t)(h >> 15) << 63;
    const unsigned e = (h >> 10) & 31u, m = h & 1023u;
    if (e == 0) {   // zero or denormal: m * 2^-24
        if (m == 0) return from_bits(sign);
        int top = 9;
        while (!((m >> top) & 1u)) top--;
        const uint64_t frac = ((uint64_t)m << (52 - top)) & ((1ull << 52) - 1ull);   // the leading 1 becomes the hidden bit
        return from_bits(sign | ((uint64_t)(1023 - 24 + top) << 52) | frac);
    }
    return from_bits(sign | ((uint64_t)(e - 15 + 1023) << 52) | ((uint64_t)m << 42));
}

int main()
{
    using tilespmv::value_half_bits;
    using tilespmv::value_halvable;
    int bad = 0, accepted = 0;
    for (unsigned h = 0; h < 65536u; h++) {
        const unsigned e = (h >> 10) & 31u, m = h & 1023u;
        if (e == 31) {   // infinity / NaN patterns: the doubles of that class are refused
            const double d = from_bits(((uint64_t)(h >> 15) << 63) | (0x7FFull << 52) | ((uint64_t)m << 42));
            if (value_halvable(d)) { printf("pattern %04x: infinity / NaN accepted\n", h); bad++; }
            continue;
        }
        const double d = decode_half(h);
        const bool want = (e == 0 && m == 0) || e != 0;   // +-0 and the normals; the denormals (e == 0, m != 0) are refused
        if (value_halvable(d) != want) { printf("pattern %04x (%.17g): halvable = %d, expected %d\n", h, d, (int)value_halvable(d), (int)want); bad++; continue; }
        if (!want) continue;
        accepted++;
        if (!tilespmv::value_narrowable(d)) { printf("pattern %04x (%.17g): a half that is no float\n", h, d); bad++; }
        if (value_half_bits(d) != h) { printf("pattern %04x (%.17g): value_half_bits = %04x\n", h, d, (unsigned)value_half_bits(d)); bad++; }
        // the two neighbouring doubles (bit pattern +- 1; next to +-0 these are the smallest fp64 denormal and the zero of the other sign's neighbour) are no halves
        const uint64_t b = to_bits(d);
        const uint64_t up = b + 1, down = (b << 1) == 0 ? (b ^ (1ull << 63)) + 1 : b - 1;
        for (const uint64_t nb : {up, down})
            if (value_halvable(from_bits(nb))) { printf("pattern %04x: neighbour %016llx accepted\n", h, (unsigned long long)nb); bad++; }
    }
    if (accepted != 2 + 2 * 30 * 1024) { printf("accepted %d patterns, expected %d\n", accepted, 2 + 2 * 30 * 1024); bad++; }
    // values the plan tests name
    const double yes[] = {6.103515625e-05, 1.0009765625, 65504.0, -0.0, -65504.0, -6.103515625e-05, 0.25, 2048.0, 9.0};
    const double no[] = {3.0517578125e-05, 5.9604644775390625e-08, 1.00048828125, 65536.0, 65504.00000000001, 0.1, 2049.0};
    for (const double v : yes) if (!value_halvable(v)) { printf("%.17g refused\n", v); bad++; }
    for (const double v : no) if (value_halvable(v)) { printf("%.17g accepted\n", v); bad++; }
    printf("%d patterns accepted, %d failures\n", accepted, bad);
    return bad ? 1 : 0;
}
