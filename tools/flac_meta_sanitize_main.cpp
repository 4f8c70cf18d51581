// The host half of the FLAC metadata (jbonsai_amd/csrc/jb_flac.cpp, jb_md5.h) under AddressSanitizer + UBSan, as a
// program of its own (tools/flac_meta_sanitize.sh builds and runs it; no GPU is touched and nothing is loaded into
// python): jb_md5_host on RFC 1321's test suite and on buffers of exactly the message's size; the chain the kernel
// runs (md5_samples) on the host over utterances packed into a slab of exactly their samples, every dword and
// sample it asks for checked against the utterance's own range, against jb_md5_host of the same bytes; the seek
// geometry's invariants; flac_plan's new fields and its bound.
#include "../jbonsai_amd/csrc/jb_host.h"

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

static int fail(const char *what, uint64_t a, uint64_t b)
{
    fprintf(stderr, "FAILED: %s at %llu, %llu\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

static std::string hex(const uint8_t d[16])
{
    char s[33];
    for (int k = 0; k < 16; k++)
        snprintf(s + 2 * k, 3, "%02x", d[k]);
    return s;
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
    // RFC 1321, A.5
    const char *msg[7] = {"", "a", "abc", "message digest", "abcdefghijklmnopqrstuvwxyz",
                          "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789",
                          "12345678901234567890123456789012345678901234567890123456789012345678901234567890"};
    const char *want[7] = {"d41d8cd98f00b204e9800998ecf8427e", "0cc175b9c0f1b6a831c399e269772661",
                           "900150983cd24fb0d6963f7d28e17f72", "f96b697d7cb7938d525a2f31aaf161d0",
                           "c3fcd3d76192e4007dfb496cca67e13b", "d174ab98d277d9f5a5611c2c9f419d9f",
                           "57edf4a22be3c955ac49da2e2107b67a"};
    uint8_t dg[16];
    for (int k = 0; k < 7; k++) {
        const size_t n = strlen(msg[k]);
        std::unique_ptr<uint8_t[]> buf(new uint8_t[n]); // exactly n bytes on the heap
        memcpy(buf.get(), msg[k], n);
        if (jb_md5_host(buf.get(), n, dg) || hex(dg) != want[k])
            return fail("RFC 1321 test suite", (uint64_t)k, n);
    }
    for (size_t n = 0; n <= 200; n++) {
        std::unique_ptr<uint8_t[]> buf(new uint8_t[n]);
        for (size_t k = 0; k < n; k++)
            buf[k] = (uint8_t)rnd();
        if (jb_md5_host(buf.get(), n, dg))
            return fail("jb_md5_host", n, 0);
    }
    // the kernel's chain over a slab of exactly the samples: utterance u starts at the prefix sum of the lengths
    const std::vector<uint64_t> lens = {0, 1, 2, 27, 28, 29, 31, 32, 33, 59, 60, 63, 64, 65, 95, 96, 97, 4095, 4096, 4097};
    size_t chains = 0;
    for (int rev = 0; rev < 2; rev++) {
        std::vector<uint64_t> ns(lens);
        if (rev)
            ns.assign(lens.rbegin(), lens.rend());
        uint64_t total = 0;
        for (uint64_t n : ns)
            total += n;
        std::unique_ptr<int16_t[]> slab(new int16_t[total]);
        for (uint64_t k = 0; k < total; k++)
            slab[k] = (int16_t)rnd();
        uint64_t off = 0;
        for (uint64_t n : ns) {
            const bool odd = (off & 1) != 0;
            const uint64_t w0 = off - (odd ? 1 : 0); // first sample of dword 0
            bool bad = false;
            const auto dword = [&](uint64_t i) {
                const uint64_t s = w0 + 2 * i; // samples s and s + 1 of the slab
                bad = bad || s + 1 > off + n - 1 || n == 0 || s + 1 >= total;
                uint32_t v;
                memcpy(&v, slab.get() + s, 4);
                return v;
            };
            const auto sample = [&](uint64_t i) {
                bad = bad || i >= n;
                return slab[off + i];
            };
            uint32_t st[4];
            jb::md5_samples(n, odd, dword, sample, st);
            uint8_t got[16];
            for (int k = 0; k < 16; k++)
                got[k] = (uint8_t)(st[k >> 2] >> (8 * (k & 3)));
            if (bad)
                return fail("md5_samples read outside its utterance", off, n);
            if (jb_md5_host(slab.get() + off, 2 * n, dg) || memcmp(got, dg, 16))
                return fail("md5_samples against jb_md5_host", off, n);
            off += n;
            chains++;
        }
    }
    // the geometry: the points cover every frame, the last one lies inside the stream, and there are at most 65,535
    size_t geoms = 0;
    for (uint32_t bs : {16u, 1152u, 4096u, 4608u})
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)bs - 1, (uint64_t)bs, (uint64_t)bs + 1,
                           (uint64_t)130 * bs + 5, (uint64_t)70000 * bs, (uint64_t)0xfffffffffull})
            for (uint32_t hz : {1u, 8000u, 22050u, 48000u, 655350u})
                for (uint32_t ms : {0u, 1u, 100u, 1000u, 10000u, 0xffffffffu}) {
                    uint32_t step = 0, pts = 0, hdr = 0;
                    if (jb_flac_seek_geometry(n, bs, hz, ms, &step, &pts, &hdr))
                        return fail("jb_flac_seek_geometry", n, bs);
                    const uint64_t nf = (n + bs - 1) / bs;
                    if (!ms || !nf) {
                        if (step || pts || hdr != 42)
                            return fail("geometry without a table", n, ms);
                    } else if (!step || !pts || pts > 65535 || (uint64_t)(pts - 1) * step >= nf ||
                               (uint64_t)pts * step < nf || hdr != 46 + 18 * pts)
                        return fail("geometry invariants", n, ms);
                    geoms++;
                }
    if (jb_flac_seek_geometry(1, 15, 48000, 1, nullptr, nullptr, nullptr) != JB_ERR_INVALID ||
        jb_flac_seek_geometry(1, 4096, 0, 1, nullptr, nullptr, nullptr) != JB_ERR_INVALID)
        return fail("geometry refusals", 0, 0);
    // the checks and the plan
    const jb_flac_meta bad_flag = {2, 0, {0, 0}}, bad_res = {1, 0, {0, 3}}, both = {JB_FLAC_MD5, 100, {0, 0}};
    jb::FlacMeta m{};
    if (jb::flac_check_meta(&bad_flag, &m) != JB_ERR_INVALID || jb::flac_check_meta(&bad_res, &m) != JB_ERR_INVALID ||
        jb::flac_check_meta(nullptr, &m) || m.flags || m.seek_interval_ms || jb::flac_check_meta(&both, &m) ||
        m.flags != JB_FLAC_MD5 || m.seek_interval_ms != 100)
        return fail("flac_check_meta", 0, 0);
    for (uint32_t bs : {16u, 4096u}) {
        const jb_flac_opts o = {bs, 8, {0, 0}};
        jb::FlacParams p{};
        if (jb::flac_check_opts(&o, &p))
            return fail("flac_check_opts", bs, 0);
        const std::vector<uint64_t> ns = {0, 1, bs, (uint64_t)bs + 1, (uint64_t)131 * bs - 11, 77777};
        const std::vector<uint32_t> hz = {48000, 8000, 22050, 16000, 8000, 44100};
        std::vector<const int16_t *> xs(ns.size(), nullptr);
        for (const jb::FlacMeta &mm : {jb::FlacMeta{0, 0, {0, 0}}, m}) {
            std::vector<jb::FlacUtt> utts;
            std::vector<jb::FlacWork> work;
            uint64_t slots = 0, bound = 0, sum = 0;
            if (jb::flac_plan(p, mm, xs.data(), ns.data(), hz.data(), ns.size(), &utts, &work, &slots, &bound))
                return fail("flac_plan", bs, mm.seek_interval_ms);
            for (size_t u = 0; u < utts.size(); u++) {
                const jb::SeekGeometry g = jb::flac_seek_geometry(ns[u], bs, hz[u], mm.seek_interval_ms);
                if (utts[u].seek_step != g.step || utts[u].n_points != g.n_points ||
                    utts[u].header_bytes != g.header_bytes || (!mm.seek_interval_ms && g.header_bytes != 42))
                    return fail("flac_plan's metadata fields", u, bs);
                sum += utts[u].header_bytes + (uint64_t)utts[u].nframes * p.slot_bytes;
            }
            if (sum != bound)
                return fail("flac_plan's bound", sum, bound);
            std::vector<uint32_t> order;
            std::vector<uint8_t> only(utts.size(), 0);
            only[1] = only[4] = 1;
            jb::flac_md5_order(utts, nullptr, &order);
            for (size_t k = 1; k < order.size(); k++)
                if (utts[order[k - 1]].n < utts[order[k]].n)
                    return fail("flac_md5_order", k, 0);
            jb::flac_md5_order(utts, &only, &order);
            if (order.size() != 2 || order[0] != 4 || order[1] != 1)
                return fail("flac_md5_order of a redo", order.size(), 0);
        }
    }
    printf("flac metadata host code: %zu chains, %zu geometries clean\n", chains, geoms);
    return 0;
}
