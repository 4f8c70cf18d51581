// The host half of IMA ADPCM (jbonsai_amd/csrc/jb_adpcm.cpp) under AddressSanitizer + UBSan, as a program of its own
// (tools/adpcm_sanitize.sh builds and runs it; no GPU is touched and nothing is loaded into python): the encoders
// and the decoder over block-boundary lengths into buffers of exactly the geometry's size, so that one byte or one
// sample too many is an error the sanitizer reports.
#include "../include/jbonsai_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace jb {
static std::string g_last;
void set_error(const std::string &s) { g_last = s; } // (the library's own lives beside the batch code)
} // namespace jb

static int fail(const char *what, uint32_t A, size_t n)
{
    fprintf(stderr, "FAILED: %s at A = %u, n = %zu\n", what, A, n);
    return 1;
}

int main()
{
    uint64_t r = 88172645463325252ull;
    auto rnd = [&] {
        r ^= r << 13;
        r ^= r >> 7;
        r ^= r << 17;
        return r;
    };
    size_t runs = 0;
    for (uint32_t A : {32u, 36u, 256u, 512u, 1024u, 8192u}) {
        const uint32_t spb = 2 * (A - 4) + 1;
        for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)8, (size_t)9, (size_t)spb - 1, (size_t)spb,
                         (size_t)spb + 1, (size_t)2 * spb + 3}) {
            for (int kind = 0; kind < 4; kind++) {
                // exactly n samples on the heap: a read past sample n - 1 is out of bounds
                std::unique_ptr<double[]> x(new double[n]);
                std::unique_ptr<int16_t[]> s(new int16_t[n]);
                for (size_t k = 0; k < n; k++) {
                    const double v = kind == 0   ? 0.0
                                     : kind == 1 ? (((k / 4) & 1) ? -40000.5 : 40000.5)
                                     : kind == 2 ? 0.01 * (double)k
                                                 : (double)(int64_t)(rnd() % 70001) - 35000.0 + 0.999;
                    x[k] = v;
                    s[k] = (int16_t)std::fmax(std::fmin(v, 32767.0), -32768.0);
                }
                uint32_t a = 0, p = 0;
                size_t nb = 0, nby = 0;
                const jb_adpcm_opts o = {A, {0, 0, 0}};
                if (jb_adpcm_geometry(8000, A, n, &a, &p, &nb, &nby) || a != A || p != spb || nby != nb * A)
                    return fail("geometry", A, n);
                std::unique_ptr<uint8_t[]> y(new uint8_t[nby]), y16(new uint8_t[nby]);
                if (jb_adpcm_encode_host(x.get(), n, 8000, &o, y.get(), nby) ||
                    jb_adpcm_encode_i16_host(s.get(), n, 8000, &o, y16.get(), nby))
                    return fail("encode", A, n);
                if (nby && memcmp(y.get(), y16.get(), nby))
                    return fail("f64 against int16", A, n);
                if (nby && jb_adpcm_encode_host(x.get(), n, 8000, &o, y.get(), nby - 1) != JB_ERR_BUFFER)
                    return fail("short buffer", A, n);
                std::unique_ptr<int16_t[]> d(new int16_t[n]);
                if (jb_adpcm_decode_host(y.get(), nby, A, n, d.get(), n))
                    return fail("decode", A, n);
                for (size_t k = 0; k < n; k += spb)
                    if (d[k] != s[k])
                        return fail("a block's first sample", A, n);
                runs++;
            }
        }
    }
    printf("adpcm host code: %zu encode/decode runs clean\n", runs);
    return 0;
}
