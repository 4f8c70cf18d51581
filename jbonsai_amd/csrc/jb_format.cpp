// jb_format.cpp -- the host half of the output sample formats: the option checks, the rules of jb_format.h over PCM
// the caller holds without a GPU (jb_format_pcm_host, what the kernel is checked against) and the WAV writer of the
// formatted bytes.
#include "jb_host.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace jb {

static_assert(kFmtF32 == JB_FMT_F32 && kFmtS16 == JB_FMT_S16 && kFmtS24 == JB_FMT_S24 && kFmtUlaw == JB_FMT_ULAW &&
                  kFmtAlaw == JB_FMT_ALAW && kDitherNone == JB_DITHER_NONE && kDitherTpdf == JB_DITHER_TPDF,
              "jb_format.h restates the header's values");

int format_check_opts(uint32_t format, uint32_t dither, const char *who)
{
    if (!format_bytes(format)) {
        set_error(std::string(who) + ": a format is JB_FMT_F32, _S16, _S24, _ULAW or _ALAW");
        return JB_ERR_INVALID;
    }
    if (dither != kDitherNone && dither != kDitherTpdf) {
        set_error(std::string(who) + ": dither is JB_DITHER_NONE or JB_DITHER_TPDF");
        return JB_ERR_INVALID;
    }
    if (dither == kDitherTpdf && format != kFmtS16 && format != kFmtS24) {
        set_error(std::string(who) + ": JB_DITHER_TPDF goes with JB_FMT_S16 and JB_FMT_S24 only");
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

template <uint32_t kFmt, bool kDither> static void format_host(const double *in, size_t n, uint64_t mseed, uint8_t *out)
{
    constexpr size_t nb = format_bytes(kFmt);
    for (size_t k = 0; k < n; k++) {
        const uint32_t w = fmt_sample<kFmt, kDither>(in[k], mseed, k);
        for (size_t j = 0; j < nb; j++)
            out[k * nb + j] = (uint8_t)(w >> (8 * j));
    }
}

} // namespace jb

using namespace jb;

extern "C" {

size_t jb_format_bytes_per_sample(uint32_t format) { return format_bytes(format); }

int jb_format_pcm_host(const double *in, size_t n, const jb_format_opts *opts, uint8_t *out, size_t cap)
{
    if (!opts) {
        set_error("jb_format_pcm_host: opts is NULL");
        return JB_ERR_INVALID;
    }
    int rc = format_check_opts(opts->format, opts->dither, "jb_format_pcm_host");
    if (rc)
        return rc;
    if (n && (!in || !out))
        return JB_ERR_INVALID;
    if (cap / format_bytes(opts->format) < n) {
        set_error("jb_format_pcm_host: the buffer is too small");
        return JB_ERR_BUFFER;
    }
    const uint64_t ms = fmt_mix(opts->seed);
    const bool d = opts->dither == kDitherTpdf;
    switch (opts->format) {
    case kFmtF32:
        format_host<kFmtF32, false>(in, n, ms, out);
        break;
    case kFmtS16:
        d ? format_host<kFmtS16, true>(in, n, ms, out) : format_host<kFmtS16, false>(in, n, ms, out);
        break;
    case kFmtS24:
        d ? format_host<kFmtS24, true>(in, n, ms, out) : format_host<kFmtS24, false>(in, n, ms, out);
        break;
    case kFmtUlaw:
        format_host<kFmtUlaw, false>(in, n, ms, out);
        break;
    default:
        format_host<kFmtAlaw, false>(in, n, ms, out);
    }
    return JB_OK;
}

void jb_format_free(uint8_t *p) { free(p); }

// RIFF/WAVE, mono: tag 1 (S16, S24), 3 (F32), 7 (mu-law), 6 (A-law); the non-PCM tags with cbSize = 0 and a fact
// chunk; a data chunk of odd length is followed by one pad byte
int jb_write_wav_formatted(const char *path, const uint8_t *bytes, size_t n_samples, uint32_t hz, uint32_t format)
{
    const size_t nb = format_bytes(format);
    if (!nb) {
        set_error("jb_write_wav_formatted: a format is JB_FMT_F32, _S16, _S24, _ULAW or _ALAW");
        return JB_ERR_INVALID;
    }
    if (!path || (!bytes && n_samples) || n_samples > (0xffffffffull - 64) / nb) {
        set_error("bad WAV arguments");
        return JB_ERR_INVALID;
    }
    const bool pcm = format == kFmtS16 || format == kFmtS24;
    const uint16_t tag = pcm ? 1 : format == kFmtF32 ? 3 : format == kFmtUlaw ? 7 : 6;
    const uint16_t ch = 1, align = (uint16_t)nb, bits = (uint16_t)(8 * nb), cb = 0;
    const uint32_t data = (uint32_t)(n_samples * nb), pad = data & 1u, fmt_len = pcm ? 16 : 18;
    const uint32_t fact_len = 4, ns = (uint32_t)n_samples, byte_rate = hz * (uint32_t)nb;
    const uint32_t riff = 4 + (8 + fmt_len) + (pcm ? 0 : 8 + fact_len) + 8 + data + pad;
    FILE *f = fopen(path, "wb");
    if (!f) {
        set_error(std::string("cannot open ") + path + ": " + strerror(errno));
        return JB_ERR_MODEL;
    }
    const uint8_t zero = 0;
    bool ok = fwrite("RIFF", 1, 4, f) == 4 && fwrite(&riff, 4, 1, f) == 1 && fwrite("WAVEfmt ", 1, 8, f) == 8 &&
              fwrite(&fmt_len, 4, 1, f) == 1 && fwrite(&tag, 2, 1, f) == 1 && fwrite(&ch, 2, 1, f) == 1 &&
              fwrite(&hz, 4, 1, f) == 1 && fwrite(&byte_rate, 4, 1, f) == 1 && fwrite(&align, 2, 1, f) == 1 &&
              fwrite(&bits, 2, 1, f) == 1; // little-endian host (x86-64)
    if (!pcm)
        ok = ok && fwrite(&cb, 2, 1, f) == 1 && fwrite("fact", 1, 4, f) == 4 && fwrite(&fact_len, 4, 1, f) == 1 &&
             fwrite(&ns, 4, 1, f) == 1;
    ok = ok && fwrite("data", 1, 4, f) == 4 && fwrite(&data, 4, 1, f) == 1 &&
         (data == 0 || fwrite(bytes, 1, data, f) == data) && (!pad || fwrite(&zero, 1, 1, f) == 1);
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        set_error(std::string("short write to ") + path);
        return JB_ERR_MODEL;
    }
    return JB_OK;
}

} // extern "C"
