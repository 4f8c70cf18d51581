// The converter's rule (include/jbonsai_amd.h, "output rate") on the host with real FMAs; no GPU.  Built with the host
// pass of hipcc and -ffp-contract=off against the built library, whose jb_resample_filter gives the taps.
//   resample_probe in_hz out_hz in.bin out.bin [n_0 n_1 ...]
// in.bin: f64 samples, the utterances of n_0, n_1, ... samples one behind the other (no lengths: the file is one
// utterance).  out.bin: each utterance's ceil(n L / M) outputs, one behind the other.  Output k of an utterance:
//   q = floor(k M / L), p = k M mod L, a = q - C + 1
//   y[k] = fma(h[p][ntaps-1], x[a + ntaps-1], ... fma(h[p][1], x[a + 1], h[p][0] * x[a]))
// in ascending j; a sample outside [0, n) is +0.0 and is multiplied and added like any other, so that the sign of a
// zero output is the device's.
#include "jbonsai_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static std::vector<double> read_all(const char *path)
{
    std::vector<double> v;
    FILE *f = fopen(path, "rb");
    if (!f)
        return v;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(double));
    if (fread(v.data(), sizeof(double), v.size(), f) != v.size())
        v.clear();
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 5) {
        fprintf(stderr, "resample_probe in_hz out_hz in.bin out.bin [lengths]\n");
        return 2;
    }
    const uint32_t in_hz = (uint32_t)strtoul(argv[1], nullptr, 10), out_hz = (uint32_t)strtoul(argv[2], nullptr, 10);
    uint32_t L = 0, M = 0, ntaps = 0;
    if (jb_resample_filter(in_hz, out_hz, &L, &M, &ntaps, nullptr, 0)) {
        fprintf(stderr, "%s\n", jb_last_error());
        return 3;
    }
    std::vector<double> h((size_t)L * ntaps);
    if (jb_resample_filter(in_hz, out_hz, nullptr, nullptr, nullptr, h.data(), h.size())) {
        fprintf(stderr, "%s\n", jb_last_error());
        return 3;
    }
    const std::vector<double> x = read_all(argv[3]);
    std::vector<size_t> lens;
    size_t total = 0;
    for (int i = 5; i < argc; i++) {
        lens.push_back((size_t)strtoull(argv[i], nullptr, 10));
        total += lens.back();
    }
    if (lens.empty()) {
        lens.push_back(x.size());
        total = x.size();
    }
    if (total != x.size()) {
        fprintf(stderr, "%s holds %zu samples, the lengths say %zu\n", argv[3], x.size(), total);
        return 2;
    }
    FILE *out = fopen(argv[4], "wb");
    if (!out)
        return 2;
    const int64_t C = ntaps / 2;
    size_t at = 0;
    for (const size_t n : lens) {
        const double *u = x.data() + at;
        at += n;
        const uint64_t n_out = ((uint64_t)n * L + M - 1) / M;
        std::vector<double> y(n_out);
        auto xin = [&](int64_t a) { return (a >= 0 && a < (int64_t)n) ? u[a] : 0.0; };
        for (uint64_t k = 0; k < n_out; k++) {
            const int64_t a = (int64_t)((k * M) / L) - C + 1;
            const double *hp = h.data() + (size_t)((k * M) % L) * ntaps;
            double acc = hp[0] * xin(a);
            for (uint32_t j = 1; j < ntaps; j++)
                acc = std::fma(hp[j], xin(a + j), acc);
            y[k] = acc;
        }
        if (fwrite(y.data(), sizeof(double), y.size(), out) != y.size())
            return 2;
    }
    return fclose(out) ? 2 : 0;
}
