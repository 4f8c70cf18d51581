#pragma once
// jb_melbank.h -- a bank of triangular filters over the n_fft / 2 + 1 bins of a frame's transform, as the filterbank
// features and the mel spectrograms hold it: each filter's weights over its support for the host, the same weights by
// bin for the kernels, the host's sum of one filter and the write of one output element.  Plain C++17.
#include "jb_rfft.h"

#include <string.h>

namespace jb {

struct MelBank {
    std::vector<double> wts;     // the filters' weights over their supports, filter after filter
    std::vector<uint32_t> first; // [n_mels] a filter's first bin with a weight above 0
    std::vector<uint32_t> count; // [n_mels] its bins (0: it covers none)
    std::vector<uint32_t> woff;  // [n_mels] its first weight in wts
    // The same weights by bin, for the kernels.  A bin lies on the rising side of at most one filter (at or below its
    // centre) and on the falling side of at most one; a filter's support is its `rise` rising bins, then its falling
    // ones
    std::vector<uint32_t> rise; // [n_mels]
    std::vector<double> wr, wf; // [K] the bin's weight in its rising / falling filter (0: none)
};

// The bank of the dense W[n_mels][K]; rising(m, k): bin k is at or below filter m's centre.  false: a bin came out on
// the same side of two filters (the by-bin form does not hold it; not expected)
template <class Rising> bool mel_bank_split(const double *W, uint32_t n_mels, uint32_t K, Rising rising, MelBank *t)
{
    t->wts.clear();
    t->first.assign(n_mels, 0);
    t->count.assign(n_mels, 0);
    t->woff.assign(n_mels, 0);
    t->rise.assign(n_mels, 0);
    t->wr.assign(K, 0.0);
    t->wf.assign(K, 0.0);
    bool ok = true;
    for (uint32_t m = 0; m < n_mels; m++) {
        // (the weights rise and fall along the bins: those above 0 are one run)
        const double *Wm = W + (size_t)m * K;
        uint32_t a = 0, b = 0;
        for (uint32_t k = 0; k < K; k++)
            if (Wm[k] > 0.0) {
                if (a == b)
                    a = k;
                b = k + 1;
            }
        t->first[m] = a;
        t->count[m] = b - a;
        t->woff[m] = (uint32_t)t->wts.size();
        t->wts.insert(t->wts.end(), Wm + a, Wm + b);
        for (uint32_t k = a; k < b; k++) {
            const bool up = rising(m, k);
            std::vector<double> &side = up ? t->wr : t->wf;
            ok = ok && side[k] == 0.0 && (up ? t->rise[m] == k - a : true);
            side[k] = Wm[k];
            t->rise[m] += up;
        }
    }
    return ok;
}

// Element `at` of a host form's output: v as it stands (f64), or rounded once to f32
inline void put_elem(uint8_t *out, size_t at, double v, bool f64)
{
    if (f64)
        memcpy(out + at * 8, &v, 8);
    else {
        const float f = (float)v;
        memcpy(out + at * 4, &f, 4);
    }
}

// Filter m over the bins' values P[0..K): its products added in ascending order
inline double mel_bank_energy(const MelBank &t, uint32_t m, const double *P)
{
    double e = 0.0;
    const double *w = t.wts.data() + t.woff[m];
    for (uint32_t i = 0; i < t.count[m]; i++)
        e += w[i] * P[t.first[m] + i];
    return e;
}

} // namespace jb
