// jb_treesearch.hip -- the per-label decision-tree search of the front half on the device.
//
// One wave per label.  The label's bytes lie in LDS, and each lane also keeps the 8 bytes that follow "its" start
// positions in registers (kTsWin).  The wave walks every (voice, model, state) tree of the flat tables
// (jb_treesearch.h) and evaluates a node's question when the walk reaches it.  Every value that steers the walk --
// the node, the question, the answer -- is the same in all 64 lanes, so the branch at a node is uniform:
//   Contains                 lanes take start positions, 64 at a time: one masked 64-bit compare for a literal of up
//                            to 8 bytes, byte by byte from LDS beyond that; the answer is a ballot
//   Prefix / Suffix / Exact  lanes take bytes of the literal; the answer is "no lane saw a mismatch"
//   Glob                     [*]core[*] with a short core and no `*` inside (every `?` pattern of an HTS question
//                            set): the masked compare with the `?` bytes masked out, at one place or at any.
//                            Anything else (a `*` inside, a long core, a label past the registers): lanes take the
//                            question's patterns, one each, through the iterative matcher of glob_match (byte-wise,
//                            `?` is one byte); the answer is a ballot
// An answer is kept for the label in two bits per (model, question) in LDS, as QuestionMemo keeps it on the host:
// the state trees of a stream ask largely the same questions.  Every lane writes the same memo word, and reads only
// what it wrote itself, so the memo needs no barrier.  Tables live in global memory: neither the number of
// questions nor the size of a pattern is bounded here (a voice set whose memo would not fit LDS runs without one;
// a question's records are taken 64 at a time, its text from registers up to 256 bytes and from the pool beyond).
// Integer work only; results leave through plain stores of lane 0.
#include "jb_host.h"
#include "jb_treesearch.h"

namespace jb {

namespace {
constexpr int kTsWaves = 4;                 // labels per workgroup
constexpr uint32_t kTsLabelLds = 1024;      // LDS bytes of a label (kTsMaxLabel + 1)
constexpr uint32_t kTsLdsLimit = 64u << 10; // dynamic LDS of a launch without raising the limit
// Start positions of a label whose next 8 bytes each lane keeps in registers (64 per register pair): a Contains
// literal of up to 8 bytes is then ONE masked 64-bit compare per 64 positions, where reading the label from LDS byte
// by byte cost an LDS round trip per byte and pattern -- most of the kernel's time, when it was measured.  Labels of
// up to 199 bytes (the longest in the repository has 167) never leave the registers
constexpr int kTsWin = 3;
static_assert(kTsMaxLabel < kTsLabelLds, "a label must fit its LDS slot");

enum : uint32_t { kGlob = 0, kContains = 1, kPrefix = 2, kSuffix = 3, kExact = 4, kAny = 5 }; // Question::Kind

__device__ inline bool any_lane(bool p) { return __ballot(p ? 1 : 0) != 0ull; }

// glob_match (jb_voice.cpp), one lane on its own; at(p) = byte p of the pattern
template <class At> __device__ inline bool ts_glob(At at, uint32_t np, const uint8_t *s, uint32_t n)
{
    uint32_t p = 0, i = 0, star = 0xffffffffu, mark = 0;
    while (i < n) {
        const uint8_t c = p < np ? at(p) : (uint8_t)0;
        if (p < np && (c == '?' || (c != '*' && c == s[i]))) {
            p++;
            i++;
        } else if (p < np && c == '*') {
            star = p++;
            mark = i;
        } else if (star != 0xffffffffu) {
            p = star + 1;
            i = ++mark;
        } else {
            return false;
        }
    }
    while (p < np && at(p) == '*')
        p++;
    return p == np;
}

__device__ inline uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The OR of question q's patterns over the label lab[0 .. L); q and the result are wave-uniform.
// A walk is a chain of dependent loads, so a question costs what its loads cost one after the other.  The text of
// a question's patterns is contiguous in the pool: the wave fetches it with ONE load, four bytes per lane (256
// bytes; a longer question reads the pool byte by byte instead), and its pattern records with one more, a record
// per lane; both are then handed round in registers.
__device__ bool ts_ask(const TsDev &d, uint32_t q, const uint8_t *lab, uint32_t L, uint32_t lane,
                       const uint64_t (&win)[kTsWin])
{
    const TsQuestion qr = d.questions[q];
    const uint32_t first = uniform(qr.first), n = uniform(qr.n);
    const uint32_t text_off = uniform(qr.text_off), text_end = text_off + uniform(qr.text_len);
    const uint32_t base4 = text_off & ~3u; // (the pool starts 16-byte aligned, and the block goes on behind it)
    const bool in_regs = text_end - base4 <= 256u;
    uint32_t words = 0;
    if (in_regs && base4 + 4u * lane < text_end)
        words = *(const uint32_t *)(d.pool + base4 + 4u * lane);
    // byte k of the pool, k wave-uniform / k per lane
    auto text_u = [&](uint32_t k) -> uint8_t {
        if (!in_regs)
            return d.pool[k];
        const uint32_t r = k - base4;
        return (uint8_t)((uint32_t)__builtin_amdgcn_readlane((int)words, (int)(r >> 2)) >> ((r & 3u) * 8u));
    };
    auto text_v = [&](uint32_t k) -> uint8_t {
        if (!in_regs)
            return d.pool[k];
        const uint32_t r = k - base4;
        return (uint8_t)((uint32_t)__shfl((int)words, (int)(r >> 2)) >> ((r & 3u) * 8u));
    };
    bool hit = false;
    for (uint32_t c0 = 0; c0 < n && !hit; c0 += 64) {
        const uint32_t cn = min(64u, n - c0);
        TsPattern mine{kAny, 0, 0};
        if (lane < cn)
            mine = d.patterns[first + c0 + lane];
        bool has_glob = false, general = false; // general: this lane's Glob pattern needs the matcher
        for (uint32_t i = 0; i < cn && !hit; i++) {
            const uint32_t kind = (uint32_t)__builtin_amdgcn_readlane((int)mine.kind, (int)i);
            const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)mine.off, (int)i);
            const uint32_t len = (uint32_t)__builtin_amdgcn_readlane((int)mine.len, (int)i);
            if (kind == kAny) {
                hit = true;
            } else if (kind == kGlob) {
                // [*]core[*] with a core of up to 8 bytes and no `*` inside -- every `?` pattern of an HTS question
                // set -- is a literal with wildcard bytes at one place, or at any: the masked compare again
                uint32_t a = 0, b = len;
                const bool lead = len > 0 && text_u(off) == '*';
                a += lead ? 1u : 0u;
                const bool trail = b > a && text_u(off + b - 1) == '*';
                b -= trail ? 1u : 0u;
                const uint32_t clen = b - a;
                bool simple = clen <= 8;
                uint64_t pat = 0, mask = 0;
                for (uint32_t j = 0; simple && j < clen; j++) {
                    const uint8_t c = text_u(off + a + j);
                    simple = c != '*';
                    if (c != '?') {
                        pat |= (uint64_t)c << (8 * j);
                        mask |= 0xffull << (8 * j);
                    }
                }
                const uint32_t nstart = L >= clen ? L - clen + 1 : 0u; // start positions the core fits at
                simple = simple && nstart <= 64u * kTsWin;
                if (!simple) {
                    has_glob = true;
                    general = general || lane == i;
                } else if (nstart && (lead || trail || nstart == 1)) {
                    // no leading `*`: the core starts the label; no trailing `*`: it ends it
                    const uint32_t smin = lead && !trail ? nstart - 1 : 0u, smax = lead ? nstart - 1 : 0u;
                    uint32_t base = 0;
#pragma unroll
                    for (int c = 0; c < kTsWin; c++)
                        if (base <= smax && !hit) {
                            const uint32_t s0 = base + lane;
                            hit = any_lane(s0 >= smin && s0 <= smax && (win[c] & mask) == pat);
                            base += 64;
                        }
                }
            } else if (kind == kContains) {
                if (L >= len) {
                    const uint32_t nstart = L - len + 1;
                    uint32_t base = 0;
                    if (len <= 8) { // win[c] of lane l: bytes [64 c + l, 64 c + l + 8) of the label
                        uint64_t pat = 0;
                        for (uint32_t j = 0; j < len; j++)
                            pat |= (uint64_t)text_u(off + j) << (8 * j);
                        const uint64_t mask = len == 8 ? ~0ull : (1ull << (8 * len)) - 1;
#pragma unroll
                        for (int c = 0; c < kTsWin; c++)
                            if (base < nstart && !hit) {
                                hit = any_lane(base + lane < nstart && (win[c] & mask) == pat);
                                base += 64;
                            }
                    }
                    for (; base < nstart && !hit; base += 64) {
                        const uint32_t s = base + lane;
                        bool ok = s < nstart;
                        for (uint32_t j = 0; j < len; j++) {
                            const uint8_t c = text_u(off + j);
                            ok = ok && lab[s + j] == c;
                        }
                        hit = any_lane(ok);
                    }
                }
            } else { // Prefix, Suffix, Exact: the literal against one place of the label
                const bool fits = kind == kExact ? L == len : L >= len;
                if (fits) {
                    const uint32_t at = kind == kSuffix ? L - len : 0u;
                    bool bad = false;
                    for (uint32_t j0 = 0; j0 < len; j0 += 64) { // (every lane takes part in the exchange)
                        const uint32_t j = j0 + lane;
                        const uint8_t c = text_v(off + min(j, len - 1));
                        bad = bad || (j < len && lab[at + j] != c);
                    }
                    hit = !any_lane(bad);
                }
            }
        }
        if (!hit && has_glob) { // the chunk's Glob patterns, one per lane
            bool ok = false;
            if (lane < cn && general) {
                const uint8_t *__restrict__ pat = d.pool + mine.off;
                if (mine.len <= 16) { // the pattern into two registers (independent loads), then no memory in the loop
                    uint64_t lo = 0, hi = 0;
#pragma unroll
                    for (uint32_t k = 0; k < 16; k++) {
                        const uint64_t b = k < mine.len ? pat[k] : 0;
                        if (k < 8)
                            lo |= b << (8 * k);
                        else
                            hi |= b << (8 * (k - 8));
                    }
                    ok = ts_glob([&](uint32_t p) { return (uint8_t)((p < 8 ? lo >> (8 * p) : hi >> (8 * (p - 8))) & 0xff); },
                                 mine.len, lab, L);
                } else {
                    ok = ts_glob([&](uint32_t p) { return pat[p]; }, mine.len, lab, L);
                }
            }
            hit = any_lane(ok);
        }
    }
    return hit;
}

// memo: two bits per question, 0 = not asked, 2 = no, 3 = yes
__device__ inline bool ts_ask_memo(const TsDev &d, uint32_t q, const uint8_t *lab, uint32_t L, uint32_t lane,
                                   uint32_t *memo, const uint64_t (&win)[kTsWin])
{
    if (!memo)
        return ts_ask(d, q, lab, L, lane, win);
    const uint32_t w = memo[q >> 4], sh = (q & 15u) * 2u;
    const uint32_t have = (w >> sh) & 3u;
    if (have)
        return have == 3u;
    const bool yes = ts_ask(d, q, lab, L, lane, win);
    memo[q >> 4] = w | ((yes ? 3u : 2u) << sh);
    return yes;
}

__global__ __launch_bounds__(kTsWaves * 64) void k_tree_search(TsDev d, const uint8_t *__restrict__ slab,
                                                                const uint32_t *__restrict__ off, uint32_t n_labels,
                                                                int32_t *__restrict__ tree_pos,
                                                                int32_t *__restrict__ pdf_index,
                                                                uint8_t *__restrict__ gv_on)
{
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t per_wave = kTsLabelLds / 4 + d.memo_words;
    uint8_t *lab = (uint8_t *)(lds + wave * per_wave);
    uint32_t *memo = d.memo_words ? lds + wave * per_wave + kTsLabelLds / 4 : nullptr;
    const uint32_t label = blockIdx.x * kTsWaves + wave;
    uint32_t L = 0;
    if (label < n_labels) {
        const uint32_t o = off[label];
        L = min(off[label + 1] - o, kTsMaxLabel);
        for (uint32_t j = lane; j < L; j += 64)
            lab[j] = slab[o + j];
        for (uint32_t j = lane; j < d.memo_words; j += 64)
            memo[j] = 0;
    }
    __syncthreads(); // the label's bytes and the cleared memo, written by other lanes
    if (label >= n_labels)
        return;
    uint64_t win[kTsWin];
#pragma unroll
    for (int c = 0; c < kTsWin; c++) {
        uint64_t w = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t at = 64u * c + lane + k;
            w |= (uint64_t)(at < L ? lab[at] : (uint8_t)0) << (8 * k);
        }
        win[c] = w;
    }
    const uint32_t entries = d.nv * d.nkind * d.nstate;
    int32_t *tp_out = tree_pos ? tree_pos + (size_t)label * entries : nullptr; // null: positions are not wanted
    int32_t *pi_out = pdf_index + (size_t)label * entries;
    for (uint32_t m = 0; m < d.nv * d.nkind; m++) {
        const TsModel mod = d.models[m];
        const bool duration = m % d.nkind == 0;
        for (uint32_t s = 0; s < d.nstate; s++) {
            const uint32_t e = m * d.nstate + s;
            int32_t tp = -1, pi = 0;
            if (!(duration && s > 0) && mod.n_trees != 0) {
                tp = d.state_tree[e];
                const TsTree tr = d.trees[mod.tree0 + (uint32_t)(tp < 0 ? 0 : tp)];
                if (tr.root < 0) {
                    pi = tr.leaf;
                } else {
                    int32_t i = 0;
                    for (uint32_t step = 0; step < tr.n_nodes; step++) {
                        const TsNode n = d.nodes[(size_t)tr.root + (size_t)i];
                        const bool yes = ts_ask_memo(d, (uint32_t)n.question, lab, L, lane, memo, win);
                        // (the same value in every lane; said so, the walk stays on the scalar unit)
                        const int32_t next = __builtin_amdgcn_readfirstlane(yes ? n.yes : n.no);
                        if (next < 0) {
                            pi = -next;
                            break;
                        }
                        i = next;
                    }
                }
            }
            if (lane == 0) {
                if (tp_out)
                    tp_out[e] = tp;
                pi_out[e] = pi;
            }
        }
    }
    const bool off_hit = ts_ask_memo(d, d.gv_question, lab, L, lane, memo, win);
    if (lane == 0)
        gv_on[label] = off_hit ? 0 : 1;
}
} // namespace

uint32_t tree_search_memo_words(size_t n_questions)
{
    const size_t words = (n_questions + 15) / 16;
    return (kTsLabelLds + words * 4) * kTsWaves <= kTsLdsLimit ? (uint32_t)words : 0u;
}

hipError_t launch_tree_search(const TsDev &d, const uint8_t *slab, const uint32_t *off, uint32_t n_labels,
                              int32_t *tree_pos, int32_t *pdf_index, uint8_t *gv_on, hipStream_t stream)
{
    if (n_labels == 0)
        return hipSuccess;
    const size_t lds = (size_t)kTsWaves * (kTsLabelLds + (size_t)d.memo_words * 4);
    hipLaunchKernelGGL(k_tree_search, dim3((n_labels + kTsWaves - 1) / kTsWaves), dim3(kTsWaves * 64), lds, stream, d,
                       slab, off, n_labels, tree_pos, pdf_index, gv_on);
    return hipGetLastError();
}

} // namespace jb
