// Probes of the packed real transform, the mel bank and the table images (jbonsai_amd/csrc/jb_rfft.h, jb_melbank.h,
// jb_host.h) as JSON; host-only, linked against the built library for the stages' tables.  Doubles are printed as their
// 64 bits.  argv[1]:
//   power N            stdin: N samples as hex floats.  The M + 1 powers of the frame by the generic path
//                      (rfft_frame_power: the schedule of rfft_plan) and, where N is a power of two, by the stage-indexed
//                      radix-2 path (bit-reversed store, rfft_stage_butterfly, rfft_untangle): {"generic": [], "stage": []}
//   fbank hz n_mels n_fft          the dense filterbank's entries above 0 and the bank fbank_tables splits it into
//   mel hz N W H n_mels slaney     the same of mel_filterbank and mel_tables
//   words              every class cache with a few classes: words() and the size of the image bind made
#include "jb_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace jb;

static unsigned long long bits(double v)
{
    unsigned long long u;
    memcpy(&u, &v, 8);
    return u;
}
static void list_bits(const char *key, const std::vector<double> &v, const char *end)
{
    printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); i++)
        printf("%s%llu", i ? ", " : "", bits(v[i]));
    printf("]%s", end);
}
static void list_u32(const char *key, const std::vector<uint32_t> &v, const char *end)
{
    printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); i++)
        printf("%s%u", i ? ", " : "", v[i]);
    printf("]%s", end);
}

static int power(uint32_t N)
{
    std::vector<double> x(N);
    for (double &v : x) {
        std::string tok;
        if (!(std::cin >> tok))
            return 2;
        v = strtod(tok.c_str(), nullptr);
    }
    const uint32_t M = N / 2;
    const RfftPlan p = rfft_plan(N);
    std::vector<double> re(M + 1, 0.0), im(M + 1, 0.0);
    rfft_frame_power(p, [&](uint32_t i) { return x[i]; }, re.data(), im.data());
    printf("{");
    list_bits("generic", re, ", ");
    std::vector<double> sr, si;
    if (!(N & (N - 1))) {
        uint32_t log2m = 0;
        while ((1u << log2m) < M)
            log2m++;
        sr.assign(M + 1, 0.0);
        si.assign(M + 1, 0.0);
        for (uint32_t j = 0; j < M; j++) {
            uint32_t r = 0;
            for (uint32_t b = 0; b < log2m; b++)
                r |= ((j >> b) & 1u) << (log2m - 1 - b);
            sr[r] = x[2 * j];
            si[r] = x[2 * j + 1];
        }
        for (uint32_t s = 0; s < log2m; s++)
            for (uint32_t j = 0; j < M / 2; j++)
                rfft_stage_butterfly(sr.data(), si.data(), p.tw.data(), log2m, s, j);
        for (uint32_t k = 0; k <= M / 2; k++)
            rfft_untangle(sr.data(), si.data(), p.tw.data(), M, k);
    }
    list_bits("stage", sr, "}\n");
    return 0;
}

static void bank_out(const std::vector<double> &W, uint32_t n_mels, uint32_t K, const MelBank &b, bool ok)
{
    printf("{\"ok\": %s, \"K\": %u, \"W\": [", ok ? "true" : "false", K);
    for (uint32_t m = 0; m < n_mels; m++) {
        printf("%s[", m ? ", " : "");
        bool first = true;
        for (uint32_t k = 0; k < K; k++)
            if (W[(size_t)m * K + k] != 0.0) {
                printf("%s[%u, %llu]", first ? "" : ", ", k, bits(W[(size_t)m * K + k]));
                first = false;
            }
        printf("]");
    }
    printf("],\n ");
    list_u32("first", b.first, ", ");
    list_u32("count", b.count, ", ");
    list_u32("woff", b.woff, ", ");
    list_u32("rise", b.rise, ",\n ");
    list_bits("wts", b.wts, ",\n ");
    list_bits("wr", b.wr, ",\n ");
    list_bits("wf", b.wf, "}\n");
}

static int fbank(char **a)
{
    FbankOpts o{};
    o.win_us = 25000, o.hop_us = 10000;
    const uint32_t hz = (uint32_t)atoi(a[0]);
    o.n_mels = (uint32_t)atoi(a[1]);
    o.n_fft = (uint32_t)atoi(a[2]);
    FbankGeom g{};
    if (!fbank_geometry_quiet(o, hz, &g))
        return 2;
    const uint32_t K = g.n_fft / 2 + 1;
    std::vector<double> W((size_t)g.n_mels * K);
    fbank_filterbank(g, hz, W.data());
    FbankTables t;
    const bool ok = fbank_tables(g, hz, o.window, &t);
    bank_out(W, g.n_mels, K, t.bank, ok);
    return 0;
}

static int mel(char **a)
{
    MelOpts o{};
    const uint32_t hz = (uint32_t)atoi(a[0]);
    o.n_fft = (uint32_t)atoi(a[1]);
    o.win_length = (uint32_t)atoi(a[2]);
    o.hop_length = (uint32_t)atoi(a[3]);
    o.n_mels = (uint32_t)atoi(a[4]);
    o.mel_scale = o.norm = atoi(a[5]) ? 1 : 0;
    MelGeom g{};
    if (!mel_geometry_quiet(o, hz, &g))
        return 2;
    const uint32_t K = g.n_fft / 2 + 1;
    std::vector<double> W((size_t)g.n_mels * K);
    mel_filterbank(g, hz, o.mel_scale, o.norm, W.data());
    MelTables t;
    const bool ok = mel_tables(g, hz, o, &t);
    bank_out(W, g.n_mels, K, t.bank, ok);
    return 0;
}

// every pointer of a class lies in the image: [base, base + words doubles)
static bool inside(const void *p, const double *base, size_t words)
{
    return !p || ((const char *)p >= (const char *)base && (const char *)p < (const char *)(base + words));
}

static int words()
{
    static double base[1]; // (an address to bind against; nothing is read through it)
    std::vector<double> image;
    uint32_t cls = 0;
    FbankOpts fo{};
    fo.win_us = 25000, fo.hop_us = 10000, fo.n_mels = 23;
    FbankClasses fb;
    for (uint32_t hz : {8000u, 16000u, 48000u, 16000u})
        if (fb.find(fo, hz, "rfft_probe", &cls))
            return 2;
    std::vector<FbankClass> fc;
    fb.bind(fo, base, &image, &fc);
    bool in = true;
    for (const FbankClass &c : fc)
        in = in && inside(c.win, base, image.size()) && inside(c.tw, base, image.size()) &&
             inside(c.wr, base, image.size()) && inside(c.wf, base, image.size()) &&
             inside(c.first, base, image.size()) && inside(c.count, base, image.size()) &&
             inside(c.rise + fo.n_mels - 1, base, image.size());
    printf("{\"fbank\": [%zu, %zu, %zu, %s],\n", fb.words(), image.size(), fc.size(), in ? "true" : "false");
    MelOpts mo{};
    mo.n_fft = 400, mo.hop_length = 160, mo.n_mels = 80, mo.mel_scale = mo.norm = 1;
    MelClasses ml;
    for (uint32_t hz : {16000u, 22050u, 16000u})
        if (ml.find(mo, hz, "rfft_probe", &cls))
            return 2;
    std::vector<MelClass> mc;
    ml.bind(mo, base, &image, &mc);
    in = true;
    for (const MelClass &c : mc)
        in = in && inside(c.win, base, image.size()) && inside(c.tws + mo.n_fft / 2 - 1, base, image.size()) &&
             inside(c.rev, base, image.size()) && inside(c.rise + mo.n_mels - 1, base, image.size());
    printf(" \"melspec\": [%zu, %zu, %zu, %s],\n", ml.words(), image.size(), mc.size(), in ? "true" : "false");
    FirClasses fi;
    std::vector<double> taps(5000);
    for (size_t k = 0; k < taps.size(); k++)
        taps[k] = 1.0 / (double)(k + 1);
    for (uint32_t K : {8u, 300u, 5000u, 300u})
        fi.find(FirSpec{taps.data(), K, 16000, K / 2, 0});
    std::vector<FirClass> ic;
    fi.bind(base, &image, &ic);
    in = true;
    for (const FirClass &c : ic)
        in = in && inside(c.h + c.K - 1, base, image.size()) && inside(c.H, base, image.size()) &&
             (!c.tw || inside(c.tw + c.n_fft + 1, base, image.size()));
    printf(" \"fir\": [%zu, %zu, %zu, %s]}\n", fi.words(), image.size(), ic.size(), in ? "true" : "false");
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "power" && argc == 3)
        return power((uint32_t)atoi(argv[2]));
    if (mode == "fbank" && argc == 5)
        return fbank(argv + 2);
    if (mode == "mel" && argc == 8)
        return mel(argv + 2);
    if (mode == "words" && argc == 2)
        return words();
    fprintf(stderr, "bad arguments\n");
    return 2;
}
