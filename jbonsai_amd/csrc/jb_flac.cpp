// jb_flac.cpp -- the host half of FLAC output: the option and metadata checks, the frame-header rate codes, the
// lists of a batch of streams (flac_plan: what jb_flac.hip's kernels walk), and the rules of jb_md5.h on the host
// without a GPU (jb_md5_host, jb_flac_seek_geometry: what the kernels are checked against).
#include "jb_host.h"

#include <algorithm>
#include <string.h>

namespace jb {

static_assert(sizeof(FlacMeta) == sizeof(jb_flac_meta) && offsetof(FlacMeta, flags) == offsetof(jb_flac_meta, flags) &&
                  offsetof(FlacMeta, seek_interval_ms) == offsetof(jb_flac_meta, seek_interval_ms) &&
                  offsetof(FlacMeta, reserved) == offsetof(jb_flac_meta, reserved) && kFlacMetaMd5 == JB_FLAC_MD5,
              "jb_md5.h restates the header's metadata request");

uint32_t flac_slot_bytes(uint32_t bs) { return ((16u + 1u + 2u * bs + 2u + 3u) & ~3u) + 4u; }

int flac_check_opts(const jb_flac_opts *o, FlacParams *p)
{
    FlacParams r{};
    r.block_size = kFlacDefaultBlock;
    r.max_order = kFlacDefaultLpc;
    if (o) {
        if (o->reserved[0] || o->reserved[1]) {
            set_error("jb_flac_opts: reserved fields must be 0");
            return JB_ERR_INVALID;
        }
        if (o->block_size && (o->block_size < 16 || o->block_size > kFlacMaxBlock)) {
            set_error("jb_flac_opts: block_size must be 16..4608 (0: 4096)");
            return JB_ERR_INVALID;
        }
        if (o->max_lpc_order > kFlacMaxLpc) {
            set_error("jb_flac_opts: max_lpc_order must be 0..12");
            return JB_ERR_INVALID;
        }
        if (o->block_size)
            r.block_size = o->block_size;
        // zeros: the defaults; a block size alone keeps the default order (max_lpc_order 0 with a block size: none)
        if (o->block_size || o->max_lpc_order)
            r.max_order = o->max_lpc_order;
    }
    r.slot_bytes = flac_slot_bytes(r.block_size);
    if (p)
        *p = r;
    return JB_OK;
}

int flac_rate_code(uint32_t hz, uint32_t *code, uint32_t *bits, uint32_t *val)
{
    static const uint32_t table[][2] = {{88200, 1}, {176400, 2}, {192000, 3}, {8000, 4},   {16000, 5}, {22050, 6},
                                        {24000, 7}, {32000, 8},   {44100, 9},  {48000, 10}, {96000, 11}};
    *bits = 0;
    *val = 0;
    for (const auto &e : table)
        if (e[0] == hz) {
            *code = e[1];
            return JB_OK;
        }
    if (hz % 1000 == 0 && hz / 1000 <= 255 && hz) {
        *code = 12, *bits = 8, *val = hz / 1000;
    } else if (hz && hz <= 65535) {
        *code = 13, *bits = 16, *val = hz;
    } else if (hz && hz % 10 == 0 && hz / 10 <= 65535) {
        *code = 14, *bits = 16, *val = hz / 10;
    } else {
        set_error("FLAC: a rate of " + std::to_string(hz) + " Hz has no frame-header code");
        return JB_ERR_UNSUPPORTED;
    }
    return JB_OK;
}

int flac_plan(const FlacParams &p, const FlacMeta &meta, const int16_t *const *x, const uint64_t *n,
              const uint32_t *hz, size_t n_utts, std::vector<FlacUtt> *utts, std::vector<FlacWork> *work,
              uint64_t *slot_bytes, uint64_t *out_bound)
{
    utts->assign(n_utts, FlacUtt{});
    work->clear();
    uint64_t frames = 0, slots = 0, bound = 0;
    for (size_t u = 0; u < n_utts; u++) {
        FlacUtt &w = (*utts)[u];
        int rc = flac_rate_code(hz[u], &w.rate_code, &w.rate_bits, &w.rate_val);
        if (rc)
            return rc;
        if (n[u] > 0xfffffffffull) {
            set_error("FLAC: an utterance longer than 2^36 samples");
            return JB_ERR_UNSUPPORTED;
        }
        w.x = x[u];
        w.n = n[u];
        w.hz = hz[u];
        w.nframes = (uint32_t)((n[u] + p.block_size - 1) / p.block_size);
        w.frame0 = frames;
        const SeekGeometry g = flac_seek_geometry(n[u], p.block_size, hz[u], meta.seek_interval_ms);
        w.seek_step = g.step;
        w.n_points = g.n_points;
        w.header_bytes = g.header_bytes;
        w.slots = (uint8_t *)(uintptr_t)slots; // an offset until the slab exists (flac_bind)
        for (uint32_t f = 0; f < w.nframes; f++)
            work->push_back(FlacWork{(uint32_t)u, f});
        frames += w.nframes;
        slots += (uint64_t)w.nframes * p.slot_bytes;
        bound += w.header_bytes + (uint64_t)w.nframes * p.slot_bytes;
    }
    *slot_bytes = slots;
    *out_bound = bound;
    return JB_OK;
}

void flac_bind(std::vector<FlacUtt> *utts, uint8_t *slots)
{
    for (auto &w : *utts)
        w.slots = slots + (uintptr_t)w.slots;
}

int flac_check_meta(const jb_flac_meta *meta, FlacMeta *m)
{
    FlacMeta r{};
    if (meta) {
        if (meta->flags & ~kFlacMetaMd5) {
            set_error("jb_flac_meta: unknown flag bits (JB_FLAC_MD5 is the only one)");
            return JB_ERR_INVALID;
        }
        if (meta->reserved[0] || meta->reserved[1]) {
            set_error("jb_flac_meta: reserved fields must be 0");
            return JB_ERR_INVALID;
        }
        r.flags = meta->flags;
        r.seek_interval_ms = meta->seek_interval_ms;
    }
    if (m)
        *m = r;
    return JB_OK;
}

void flac_md5_order(const std::vector<FlacUtt> &utts, const std::vector<uint8_t> *only, std::vector<uint32_t> *order)
{
    order->clear();
    for (size_t u = 0; u < utts.size(); u++)
        if (!only || (*only)[u])
            order->push_back((uint32_t)u);
    std::stable_sort(order->begin(), order->end(), [&](uint32_t a, uint32_t b) { return utts[a].n > utts[b].n; });
}

} // namespace jb

using namespace jb;

extern "C" {

int jb_md5_host(const void *data, size_t n_bytes, uint8_t digest[16])
{
    if (!digest || (n_bytes && !data))
        return JB_ERR_INVALID;
    const uint8_t *p = (const uint8_t *)data;
    uint32_t st[4] = {kMd5Init[0], kMd5Init[1], kMd5Init[2], kMd5Init[3]};
    // byte i of the padded message, the count apart: the data, one 0x80, zeros
    const auto byte_at = [&](uint64_t i) -> uint32_t { return i < n_bytes ? p[i] : i == n_bytes ? 0x80u : 0u; };
    const uint64_t nb = ((uint64_t)n_bytes + 9 + 63) / 64, bits = 8 * (uint64_t)n_bytes;
    for (uint64_t k = 0; k < nb; k++) {
        uint32_t m[16];
        for (int j = 0; j < 16; j++) {
            const uint64_t i = 64 * k + 4 * (uint64_t)j;
            m[j] = byte_at(i) | (byte_at(i + 1) << 8) | (byte_at(i + 2) << 16) | (byte_at(i + 3) << 24);
        }
        if (k == nb - 1) {
            m[14] = (uint32_t)bits;
            m[15] = (uint32_t)(bits >> 32);
        }
        md5_block(st, m);
    }
    for (int k = 0; k < 16; k++)
        digest[k] = (uint8_t)(st[k >> 2] >> (8 * (k & 3)));
    return JB_OK;
}

int jb_flac_seek_geometry(uint64_t n_samples, uint32_t block_size, uint32_t hz, uint32_t seek_interval_ms,
                          uint32_t *step_frames, uint32_t *n_points, uint32_t *header_bytes)
{
    const jb_flac_opts o = {block_size, 0, {0, 0}}; // (0: the default block size)
    FlacParams p{};
    int rc = flac_check_opts(&o, &p);
    if (rc)
        return rc;
    if (n_samples > 0xfffffffffull || hz == 0) {
        set_error("jb_flac_seek_geometry: at most 2^36 - 1 samples, at a rate above 0");
        return JB_ERR_INVALID;
    }
    const SeekGeometry g = flac_seek_geometry(n_samples, p.block_size, hz, seek_interval_ms);
    if (step_frames)
        *step_frames = g.step;
    if (n_points)
        *n_points = g.n_points;
    if (header_bytes)
        *header_bytes = g.header_bytes;
    return JB_OK;
}

} // extern "C"
