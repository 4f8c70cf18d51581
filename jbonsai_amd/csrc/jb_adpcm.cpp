// jb_adpcm.cpp -- the host half of IMA ADPCM: the option check, the geometry, the rules of jb_adpcm.h over PCM the
// caller holds without a GPU (jb_adpcm_encode_host, what the kernel is checked against), the decoder and the WAV
// writer of the blocks.
#include "jb_host.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(sizeof(AdpcmOpts) == sizeof(jb_adpcm_opts) &&
                  offsetof(AdpcmOpts, block_align) == offsetof(jb_adpcm_opts, block_align) &&
                  offsetof(AdpcmOpts, reserved) == offsetof(jb_adpcm_opts, reserved),
              "jb_adpcm.h restates the header's options");

int adpcm_check_opts(const AdpcmOpts *opts, const char *who)
{
    if (!opts) {
        set_error(std::string(who) + ": opts is NULL");
        return JB_ERR_INVALID;
    }
    if (!adpcm_align_ok(opts->block_align)) {
        set_error(std::string(who) + ": block_align is 0 (by the rate) or a multiple of 4 in 32..8192");
        return JB_ERR_INVALID;
    }
    if (opts->reserved[0] || opts->reserved[1] || opts->reserved[2]) {
        set_error(std::string(who) + ": reserved must be 0");
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

namespace {

struct StepTable {
    int32_t t[kAdpcmSteps];
    StepTable()
    {
        for (uint32_t i = 0; i < kAdpcmSteps; i++)
            t[i] = adpcm_step_of(i);
    }
    int32_t operator[](int32_t i) const { return t[i]; }
};
const StepTable g_steps;

inline int32_t sample_of(const double *in, size_t k) { return fmt_quant<false>(in[k], -32768.0, 32767.0, 0, 0); }
inline int32_t sample_of(const int16_t *in, size_t k) { return in[k]; }

// n > 0 samples into ceil(n / spb) blocks of A bytes
template <class T> void encode(const T *in, size_t n, uint32_t A, uint8_t *out)
{
    const uint32_t spb = adpcm_spb(A);
    const size_t nb = (size_t)adpcm_blocks(n, A);
    for (size_t blk = 0; blk < nb; blk++) {
        const size_t k0 = blk * spb;
        auto b = [&](uint32_t k) { return sample_of(in, k0 + k < n ? k0 + k : n - 1); };
        uint8_t *y = out + blk * A;
        int32_t pred = b(0), d = 0;
        for (uint32_t k = 1; k <= 8; k++)
            d += abs(b(k) - b(k - 1));
        int32_t idx = adpcm_start_index(d >> 3, g_steps);
        y[0] = (uint8_t)pred;
        y[1] = (uint8_t)(pred >> 8);
        y[2] = (uint8_t)idx;
        y[3] = 0;
        for (uint32_t j = 0; j < A - 4; j++) {
            const uint32_t lo = adpcm_code(b(2 * j + 1), g_steps[idx], pred, idx);
            const uint32_t hi = adpcm_code(b(2 * j + 2), g_steps[idx], pred, idx);
            y[4 + j] = (uint8_t)(lo | (hi << 4));
        }
    }
}

template <class T>
int encode_entry(const T *in, size_t n, uint32_t hz, const jb_adpcm_opts *opts, uint8_t *out, size_t cap, const char *who)
{
    int rc = adpcm_check_opts((const AdpcmOpts *)opts, who);
    if (rc)
        return rc;
    if (n && (!in || !out))
        return JB_ERR_INVALID;
    const uint32_t A = adpcm_block_align(hz, opts->block_align);
    if (cap < adpcm_bytes(n, A)) {
        set_error(std::string(who) + ": the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (n)
        encode(in, n, A, out);
    return JB_OK;
}

} // namespace

} // namespace jb

using namespace jb;

extern "C" {

int jb_adpcm_geometry(uint32_t hz, uint32_t block_align, size_t n, uint32_t *A, uint32_t *spb, size_t *n_blocks,
                      size_t *n_bytes)
{
    const AdpcmOpts o{block_align, {0, 0, 0}};
    int rc = adpcm_check_opts(&o, "jb_adpcm_geometry");
    if (rc)
        return rc;
    const uint32_t a = adpcm_block_align(hz, block_align);
    if (A)
        *A = a;
    if (spb)
        *spb = adpcm_spb(a);
    if (n_blocks)
        *n_blocks = (size_t)adpcm_blocks(n, a);
    if (n_bytes)
        *n_bytes = (size_t)adpcm_bytes(n, a);
    return JB_OK;
}

int jb_adpcm_encode_host(const double *in, size_t n, uint32_t hz, const jb_adpcm_opts *opts, uint8_t *out, size_t cap)
{
    return encode_entry(in, n, hz, opts, out, cap, "jb_adpcm_encode_host");
}

int jb_adpcm_encode_i16_host(const int16_t *in, size_t n, uint32_t hz, const jb_adpcm_opts *opts, uint8_t *out,
                             size_t cap)
{
    return encode_entry(in, n, hz, opts, out, cap, "jb_adpcm_encode_i16_host");
}

int jb_adpcm_decode_host(const uint8_t *bytes, size_t n_bytes, uint32_t A, size_t n_samples, int16_t *out, size_t cap)
{
    if (A == 0 || !adpcm_align_ok(A)) {
        set_error("jb_adpcm_decode_host: A is a multiple of 4 in 32..8192");
        return JB_ERR_INVALID;
    }
    if (adpcm_blocks(n_samples, A) > n_bytes / A) {
        set_error("jb_adpcm_decode_host: fewer blocks than the samples need");
        return JB_ERR_INVALID;
    }
    if (cap < n_samples) {
        set_error("jb_adpcm_decode_host: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    if (n_samples && (!bytes || !out))
        return JB_ERR_INVALID;
    const uint32_t spb = adpcm_spb(A);
    for (size_t blk = 0, k = 0; k < n_samples; blk++) {
        const uint8_t *y = bytes + blk * A;
        int32_t pred = (int16_t)(uint16_t)(y[0] | (y[1] << 8));
        int32_t idx = y[2] > 88 ? 88 : y[2];
        out[k++] = (int16_t)pred;
        for (uint32_t j = 1; j < spb && k < n_samples; j++) {
            const uint8_t by = y[4 + (j - 1) / 2];
            adpcm_decode((j & 1) ? (by & 15u) : (uint32_t)(by >> 4), g_steps[idx], pred, idx);
            out[k++] = (int16_t)pred;
        }
    }
    return JB_OK;
}

void jb_adpcm_free(uint8_t *p) { free(p); }

int jb_write_wav_adpcm(const char *path, const uint8_t *bytes, size_t n_bytes, size_t n_samples, uint32_t hz,
                       uint32_t block_align)
{
    if (block_align == 0 || !adpcm_align_ok(block_align)) {
        set_error("jb_write_wav_adpcm: block_align is a multiple of 4 in 32..8192");
        return JB_ERR_INVALID;
    }
    if (!path || (!bytes && n_bytes) || n_bytes > 0xffffffffull - 64 || n_samples > 0xffffffffull ||
        n_bytes != adpcm_bytes(n_samples, block_align)) {
        set_error("bad WAV arguments");
        return JB_ERR_INVALID;
    }
    const uint16_t tag = 0x11, ch = 1, align = (uint16_t)block_align, bits = 4, cb = 2;
    const uint16_t spb = (uint16_t)adpcm_spb(block_align);
    const uint32_t data = (uint32_t)n_bytes, fmt_len = 20, fact_len = 4, ns = (uint32_t)n_samples;
    const uint32_t byte_rate = (uint32_t)((uint64_t)hz * block_align / spb);
    const uint32_t riff = 4 + (8 + fmt_len) + (8 + fact_len) + 8 + data; // (data is even: A is a multiple of 4)
    FILE *f = fopen(path, "wb");
    if (!f) {
        set_error(std::string("cannot open ") + path + ": " + strerror(errno));
        return JB_ERR_MODEL;
    }
    bool ok = fwrite("RIFF", 1, 4, f) == 4 && fwrite(&riff, 4, 1, f) == 1 && fwrite("WAVEfmt ", 1, 8, f) == 8 &&
              fwrite(&fmt_len, 4, 1, f) == 1 && fwrite(&tag, 2, 1, f) == 1 && fwrite(&ch, 2, 1, f) == 1 &&
              fwrite(&hz, 4, 1, f) == 1 && fwrite(&byte_rate, 4, 1, f) == 1 && fwrite(&align, 2, 1, f) == 1 &&
              fwrite(&bits, 2, 1, f) == 1 && fwrite(&cb, 2, 1, f) == 1 && fwrite(&spb, 2, 1, f) == 1 &&
              fwrite("fact", 1, 4, f) == 4 && fwrite(&fact_len, 4, 1, f) == 1 && fwrite(&ns, 4, 1, f) == 1 &&
              fwrite("data", 1, 4, f) == 4 && fwrite(&data, 4, 1, f) == 1 &&
              (data == 0 || fwrite(bytes, 1, data, f) == data); // little-endian host (x86-64)
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        set_error(std::string("short write to ") + path);
        return JB_ERR_MODEL;
    }
    return JB_OK;
}

} // extern "C"
