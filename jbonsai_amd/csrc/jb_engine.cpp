// jb_engine.cpp -- engine-level C ABI (include/jbonsai_amd.h, part 2).
//
// Host front half (cold, per utterance O(labels)): label lines -> per-state pdfs
// (decision-tree search, multi-voice blend) -> state durations.  Mirrors
//   Engine / Condition            src/engine.rs:31-366
//   Labels::load_from_strings     src/label.rs:35-113
//   Models::{duration,stream,gv}  src/model/mod.rs:80-156
//   VoiceSet::{new,weighted}      src/model/voice_set.rs:22-95
//   DurationEstimator             src/duration.rs:20-131
//   InterporationWeight           src/model/interporation_weight.rs:48-160
// Everything from the state level down (MLPG, GV, excitation, MLSA) is handed to
// the HIP batch (jb_batch.cpp); nothing here synthesises audio.
#include "jb_host.h"
#include "jb_treesearch.h"
#include "jb_voice.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <thread>
#include <cerrno>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/mman.h>

namespace jb {

constexpr double kDB = 0.11512925464970228;        // ln(10)/20, src/constants.rs:11
constexpr double kHalfTone = 0.05776226504666211;  // ln(2)/12,  src/constants.rs:9
constexpr double kMaxLf0 = 9.903487552536127, kMinLf0 = 2.995732273553991;

struct Condition {
    size_t sampling_frequency = 0, fperiod = 0;
    double volume = 1.0;
    std::vector<double> msd_threshold, gv_weight;
    bool phoneme_alignment = false;
    bool batch_invariant = false; // jb_engine_set_batch_invariant: JB_BATCH_SERIAL | JB_BATCH_SERIAL_GV for every batch of this engine
    bool fast_invariant = false;  // jb_engine_set_fast_invariant: JB_BATCH_INVARIANT for every batch of this engine
    uint32_t batch_flags() const
    {
        return (batch_invariant ? (JB_BATCH_SERIAL | JB_BATCH_SERIAL_GV) : 0u) | (fast_invariant ? JB_BATCH_INVARIANT : 0u);
    }
    size_t output_rate = 0;       // jb_engine_set_output_sampling_frequency: 0 = the voice's rate
    double loudness_target = NAN; // jb_engine_set_loudness_target: NaN = off
    double peak_ceiling = 0.0;    // jb_engine_set_peak_ceiling (dBFS), with a target only
    uint32_t peak_mode = JB_PEAK_SAMPLE; // jb_engine_set_peak_mode: what the ceiling bounds, with a target only
    uint32_t loudness_scope = JB_LOUDNESS_PER_UTTERANCE; // jb_engine_set_loudness_scope: what one gain covers
    jb_filter filter{};           // jb_engine_set_filter: n_sections 0 = off
    std::vector<double> fir_taps; // jb_engine_set_fir: the response's taps, copied (empty = off) ...
    uint32_t fir_hz = 0, fir_delay = 0; // ... its rate and delay
    jb_fir fir() const { return jb_fir{fir_taps.empty() ? nullptr : fir_taps.data(), (uint32_t)fir_taps.size(), fir_hz, fir_delay, 0}; }
    bool frame_on = false;        // jb_engine_set_frame_opts: a frame request for the *_fbank and *_mfcc entries ...
    jb_frame_opts frame{};        // ... as it was given
    bool room_on = false;         // jb_engine_set_room: a room is set (in the impulse response's slot) ...
    jb_room room_req{};           // ... as it was given, with its flags, seed and margin
    uint32_t room_flags = 0;
    uint64_t room_seed = 0;
    double room_margin = 0.0;
    // the room of the utterance of index k in a call (all bytes zero: none); JB_ERR_INVALID from the varied positions
    int room(uint64_t k, jb_room *out) const
    {
        *out = jb_room{};
        if (!room_on)
            return JB_OK;
        *out = room_req;
        if (room_flags & JB_ROOM_VARY)
            return jb::room_vary(room_seed, k, room_req.size, room_margin, out->source, out->mic, "jb_engine_set_room");
        return JB_OK;
    }
    std::vector<double> noise_bed; // jb_engine_set_noise: the bed's samples, copied ...
    jb_noise noise_req{};         // ... and the request as it was given (its bed pointer is not kept: noise())
    jb_noise noise() const
    {
        jb_noise r = noise_req;
        r.bed = noise_bed.empty() ? nullptr : noise_bed.data();
        return r;
    }
    bool limiter_on = false;      // jb_engine_set_limiter: a request is set ...
    jb_limiter_opts limiter{};    // ... and the request as it was given
    std::vector<jb_mix_place> mix_place; // jb_engine_set_programme_mix: each member's start and gain (empty = off) ...
    jb_mix_opts mix_opts{};              // ... and the request's options
    uint32_t tree_search = JB_SEARCH_HOST; // jb_engine_set_tree_search: where the per-label tree search runs
    double speed = 1.0;
    size_t stage = 0;
    bool use_log_gain = false;
    double alpha = 0.0, beta = 0.0, additional_half_tone = 0.0;
    // InterporationWeight
    std::vector<double> w_duration;
    std::vector<std::vector<double>> w_param, w_gv;
};

struct Engine {
    std::vector<std::shared_ptr<Voice>> voices;
    Condition cond;
    // cached static description for the state-level ABI
    jb_voice_desc desc{};
    std::vector<double> win_coef[kMaxStream];
    void refresh_desc();
    // stream pdf tables with all trees concatenated (row = tree_off[tree] + pdf-1),
    // built once, and their device copies per GPU
    struct CatTable {
        std::vector<float> rows;
        std::vector<uint32_t> tree_off;
        uint32_t n_rows = 0, row_len = 0;
    };
    mutable std::vector<CatTable> cat; // [voice * nstream + stream]
    mutable std::map<int, jb_pdf_set *> pdf_sets;
    mutable std::mutex pdf_mu;
    int pdf_set_for(int device, const jb_pdf_set **out) const;
    // device tree search (jb_engine_set_tree_search): the flat tables of the voices' trees, built at the first use,
    // their device copies per GPU (one block each), and the labels searched there so far
    struct TsDevCopy {
        void *block = nullptr;
        TsDev d{};
    };
    mutable std::unique_ptr<TsTables> ts;
    mutable std::map<int, TsDevCopy> ts_dev;
    mutable std::mutex ts_mu;
    mutable std::atomic<uint64_t> dev_searched{0};
    const TsTables &tables() const;
    int ts_dev_for(int device, TsDev *out) const;
    ~Engine()
    {
        for (auto &kv : pdf_sets)
            jb_pdf_set_free(kv.second);
        for (auto &kv : ts_dev)
            (void)hipFree(kv.second.block);
    }
};

int Engine::pdf_set_for(int device, const jb_pdf_set **out) const
{
    std::lock_guard<std::mutex> lk(pdf_mu);
    const size_t ns = std::min(voices[0]->streams.size(), (size_t)kMaxStream);
    if (cat.empty()) {
        cat.resize(voices.size() * ns);
        for (size_t v = 0; v < voices.size(); v++)
            for (size_t si = 0; si < ns; si++) {
                const Model &m = voices[v]->streams[si].stream;
                CatTable &c = cat[v * ns + si];
                c.row_len = (uint32_t)m.pdf_len;
                for (size_t t = 0; t < m.pdf.size(); t++) {
                    c.tree_off.push_back(c.n_rows);
                    c.rows.insert(c.rows.end(), m.pdf[t].begin(), m.pdf[t].end());
                    c.n_rows += (uint32_t)m.npdf[t];
                }
            }
    }
    auto it = pdf_sets.find(device);
    if (it == pdf_sets.end()) {
        std::vector<jb_pdf_table> tabs(cat.size());
        for (size_t i = 0; i < cat.size(); i++)
            tabs[i] = jb_pdf_table{cat[i].rows.data(), cat[i].n_rows, cat[i].row_len};
        jb_pdf_set *ps = nullptr;
        int rc = jb_pdf_set_create(tabs.data(), (uint32_t)voices.size(), (uint32_t)ns, device, &ps);
        if (rc)
            return rc;
        it = pdf_sets.emplace(device, ps).first;
    }
    *out = it->second;
    return JB_OK;
}

void Engine::refresh_desc()
{
    const Voice &v = *voices[0];
    memset(&desc, 0, sizeof desc);
    desc.sampling_frequency = (uint32_t)cond.sampling_frequency;
    desc.fperiod = (uint32_t)cond.fperiod;
    desc.nstream = (uint32_t)v.meta.num_streams;
    desc.stage = (uint32_t)cond.stage;
    desc.use_log_gain = cond.use_log_gain;
    desc.alpha = cond.alpha;
    desc.beta = cond.beta;
    desc.volume = cond.volume;
    for (size_t i = 0; i < v.streams.size() && i < (size_t)kMaxStream; i++) {
        const StreamModel &s = v.streams[i];
        jb_stream_desc &d = desc.stream[i];
        d.vector_length = (uint32_t)s.vector_length;
        d.num_windows = (uint32_t)s.num_windows;
        d.is_msd = s.is_msd;
        d.use_gv = s.use_gv;
        win_coef[i].clear();
        for (size_t w = 0; w < s.windows.size() && w < JB_MAX_WINDOW; w++) {
            d.win_width[w] = (uint32_t)s.windows[w].size();
            win_coef[i].insert(win_coef[i].end(), s.windows[w].begin(), s.windows[w].end());
        }
        d.win_coef = win_coef[i].data();
    }
}

// Condition::load_model (src/engine.rs:84-125)
static int load_condition(Engine &e)
{
    const Voice &v = *e.voices[0];
    Condition &c = e.cond;
    const size_t ns = (size_t)v.meta.num_streams, nv = e.voices.size();
    c.sampling_frequency = (size_t)v.meta.sampling_frequency;
    c.fperiod = (size_t)v.meta.frame_period;
    c.msd_threshold.assign(ns, 0.5);
    c.gv_weight.assign(ns, 1.0);
    for (const std::string &opt : v.streams[0].options) { // options of stream 0 only
        size_t eq = opt.find('=');
        if (eq == std::string::npos)
            continue; // "Skipped unrecognized option"
        std::string key = opt.substr(0, eq), val = opt.substr(eq + 1);
        char *end = nullptr;
        if (key == "GAMMA") {
            unsigned long g = strtoul(val.c_str(), &end, 10);
            if (val.empty() || *end) {
                set_error("Failed to parse option GAMMA");
                return JB_ERR_PARSE_OPTION;
            }
            c.stage = g;
        } else if (key == "LN_GAIN") {
            if (val == "1")
                c.use_log_gain = true;
            else if (val == "0")
                c.use_log_gain = false;
            else {
                set_error("Failed to parse option LN_GAIN");
                return JB_ERR_PARSE_OPTION;
            }
        } else if (key == "ALPHA") {
            double a = strtod(val.c_str(), &end);
            if (val.empty() || *end) {
                set_error("Failed to parse option ALPHA");
                return JB_ERR_PARSE_OPTION;
            }
            c.alpha = a;
        }
    }
    // InterporationWeight::new(nvoices, nstream): equal weights
    c.w_duration.assign(nv, 1.0 / (double)nv);
    c.w_param.assign(ns, c.w_duration);
    c.w_gv.assign(ns, c.w_duration);
    return JB_OK;
}

// VoiceSet::new metadata checks (src/model/voice_set.rs:22-42)
static int check_voiceset(const std::vector<std::shared_ptr<Voice>> &vs)
{
    if (vs.empty()) {
        set_error("No HTS voice was given.");
        return JB_ERR_MODEL;
    }
    const Voice &f = *vs[0];
    for (size_t i = 1; i < vs.size(); i++) {
        const Voice &v = *vs[i];
        bool ok = v.meta == f.meta && v.streams.size() == f.streams.size();
        for (size_t s = 0; ok && s < f.streams.size(); s++) {
            const StreamModel &a = v.streams[s], &b = f.streams[s];
            ok = a.vector_length == b.vector_length && a.num_windows == b.num_windows &&
                 a.is_msd == b.is_msd && a.use_gv == b.use_gv && a.options == b.options;
        }
        if (!ok) {
            set_error("The global metadata does not match.");
            return JB_ERR_MODEL;
        }
    }
    return JB_OK;
}

// ---- labels ----------------------------------------------------------------
struct ParsedLabels {
    std::vector<std::string> labels;
    std::vector<std::pair<double, double>> times;
};

// minimal shape check standing in for jlabel's grammar (src/label.rs:65,72)
static bool label_shape_ok(const std::string &l)
{
    return glob_match("*^*-*+*=*/A:*/B:*/C:*/D:*/E:*/F:*/G:*/H:*/I:*/J:*/K:*", l);
}

static int parse_labels(const Condition &c, const char *const *lines, size_t n, ParsedLabels &out)
{
    const double rate = (double)c.sampling_frequency / ((double)c.fperiod * 1e+7);
    for (size_t i = 0; i < n; i++) {
        if (!lines[i]) {
            set_error("null label line");
            return JB_ERR_LABEL;
        }
        std::string line(lines[i]);
        size_t s1 = line.find(' ');
        if (s1 != std::string::npos) {
            size_t s2 = line.find(' ', s1 + 1);
            if (s2 == std::string::npos) {
                set_error("Expected a fullcontext-label in " + line);
                return JB_ERR_LABEL;
            }
            char *e1 = nullptr, *e2 = nullptr;
            std::string a = line.substr(0, s1), b = line.substr(s1 + 1, s2 - s1 - 1);
            double st = strtod(a.c_str(), &e1), en = strtod(b.c_str(), &e2);
            if (a.empty() || b.empty() || *e1 || *e2) {
                set_error("Failed to parse as floating-point number");
                return JB_ERR_LABEL;
            }
            out.times.emplace_back(st * rate, en * rate);
            out.labels.push_back(line.substr(s2 + 1));
        } else if (line.empty()) {
            continue;
        } else {
            out.times.emplace_back(-1.0, -1.0);
            out.labels.push_back(line);
        }
        if (!label_shape_ok(out.labels.back())) {
            set_error("jlabel failed to parse fullcontext-label: " + out.labels.back());
            return JB_ERR_LABEL;
        }
    }
    // Labels::new (src/label.rs:83-113)
    auto &t = out.times;
    for (size_t i = 0; i < t.size(); i++) {
        if (i + 1 < t.size()) {
            if (t[i].second < 0.0 && t[i + 1].first >= 0.0)
                t[i].second = t[i + 1].first;
            else if (t[i].second >= 0.0 && t[i + 1].first < 0.0)
                t[i + 1].first = t[i].second;
        }
        if (t[i].first < 0.0)
            t[i].first = -1.0;
        if (t[i].second < 0.0)
            t[i].second = -1.0;
    }
    return JB_OK;
}

// ---- durations (src/duration.rs) -------------------------------------------
struct MV {
    double mean, vari;
};

static void estimate_duration(const MV *p, size_t n, double rho, uint32_t *d)
{
    for (size_t i = 0; i < n; i++) {
        double r = std::round(p[i].mean + rho * p[i].vari); // f64::round: half away from zero
        d[i] = (uint32_t)(r > 1.0 ? r : 1.0);
    }
}

static void estimate_with_frame_length(const MV *p, size_t n, double frame_length, uint32_t *d)
{
    double tl = std::round(frame_length);
    const size_t target = (size_t)(tl > 1.0 ? tl : 1.0);
    if (target <= n) {
        std::fill(d, d + n, 1u);
        return;
    }
    double mean = 0.0, vari = 0.0;
    for (size_t i = 0; i < n; i++) {
        mean = mean + p[i].mean;
        vari = vari + p[i].vari;
    }
    const double rho = ((double)target - mean) / vari;
    estimate_duration(p, n, rho, d);
    if (n == 0)
        return;
    size_t sum = 0;
    for (size_t i = 0; i < n; i++)
        sum += d[i];
    auto cost = [&](double dd, const MV &q) { return std::fabs(rho - (dd - q.mean) / q.vari); };
    while (sum != target) {
        const bool grow = target > sum;
        size_t best = n;
        double bc = 0.0;
        for (size_t i = 0; i < n; i++) {
            if (!grow && d[i] <= 1)
                continue;
            double c = cost((double)d[i] + (grow ? 1.0 : -1.0), p[i]);
            if (best == n || c < bc) { // first minimum wins (Iterator::min_by)
                best = i;
                bc = c;
            }
        }
        if (best == n)
            break;
        if (grow) {
            d[best]++;
            sum++;
        } else {
            d[best]--;
            sum--;
        }
    }
}

// ---- state construction ------------------------------------------------------
struct States {
    jb_state_utt utt{};
    // indexed form: pdf rows per stream and voice instead of blended Gaussians
    jb_index_utt iutt{};
    std::vector<uint32_t> rows[kMaxStream][JB_MAX_VOICES];
    std::vector<double> weights[kMaxStream];
    std::vector<uint32_t> dur;
    std::vector<double> dur_pdf; // [S][2]: Models::duration (model/mod.rs:80-92), the blended (mean, variance) the durations come from
    std::vector<double> mean[kMaxStream], var[kMaxStream], msd[kMaxStream], gvm[kMaxStream],
        gvv[kMaxStream];
    std::vector<uint8_t> gsw[kMaxStream];
};

// VoiceSet::weighted (voice_set.rs:80-95): first*w0, then += w_i * param_i, in order; get(v) = voice v's parameter.
template <class F>
static void blend(const Engine &e, const std::vector<double> &w, size_t len, double *out, F get)
{
    const float *p0 = get((size_t)0);
    for (size_t k = 0; k < len; k++)
        out[k] = (double)p0[k] * w[0];
    for (size_t v = 1; v < e.voices.size(); v++) {
        const float *p = get(v);
        for (size_t k = 0; k < len; k++)
            out[k] += w[v] * (double)p[k];
    }
}

// Model::get_parameter from a search result: the row of (tree position, 1-based pdf index)
static const float *pdf_row(const Model &m, int tp, int pi)
{
    if (tp < 0 || pi < 1 || pi > m.npdf[(size_t)tp])
        throw ModelError("index not found"); // reference: todo!() (voice/model.rs:76-79)
    return m.pdf[(size_t)tp].data() + (size_t)(pi - 1) * (size_t)m.pdf_len;
}

// Runs fn(lo, hi) over [0, n) in `nt` contiguous pieces on host threads (in the calling thread when nt == 1);
// a ModelError thrown by a piece is rethrown here.  The per-label work of the front half (tree searches with
// string-predicate questions, pdf blend) is independent per label and read-only on the engine.
template <class F> static void parallel_labels(size_t n, unsigned nt, F fn)
{
    nt = (unsigned)std::min<size_t>(nt ? nt : 1u, std::max<size_t>(n / 32, 1)); // at least 32 labels per thread
    if (nt <= 1) {
        fn((size_t)0, n);
        return;
    }
    std::vector<std::string> errs(nt);
    std::vector<uint8_t> failed(nt, 0);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; t++)
        pool.emplace_back([&, t] {
            try {
                fn(n * t / nt, n * (t + 1) / nt);
            } catch (const ModelError &ex) {
                failed[t] = 1;
                errs[t] = ex.what();
            }
        });
    for (auto &th : pool)
        th.join();
    for (unsigned t = 0; t < nt; t++)
        if (failed[t])
            throw ModelError(errs[t]);
}

// label_threads: host threads for the per-label work of ONE utterance (1 inside jb_synthesize_batch, whose
// workers already take an utterance each; several for the single-utterance entries, where a 1,456-label text
// otherwise spends 15-20 ms in tree searches before the device sees anything)
// worker threads of the front half: JB_HOST_THREADS, default min(16, cores)
static unsigned host_threads_default()
{
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt ? std::min(nt, 16u) : 1u;
    if (const char *ev = getenv("JB_HOST_THREADS"))
        nt = (unsigned)std::max(1, atoi(ev));
    return nt;
}

// The front half of one utterance goes in three steps: parse (label lines -> labels and times), search (every
// label's trees -> FrontUtt::tp / pi / gv_on) and finish (pdf rows or blended Gaussians, durations, GV).  The search
// runs on the host threads -- then inside the finish step's one pass over the labels, label by label, as it always
// has -- or beforehand on the device (device_tree_search), which fills the same block.
struct FrontUtt {
    ParsedLabels pl;
    // per label [nv][1 + nstream][nstate]: what Model::get_index returns (tree position, 1-based pdf index), laid
    // out as ts_walk_label's; gv_on per label: !gv_off.test(label)
    std::vector<int32_t> tp, pi;
    std::vector<uint8_t> gv_on;
    // the block as the device filled it: the utterance's part of its request's DeviceIndex (null: not searched yet)
    // (dev_tp: [entries], the same for every label)
    const int32_t *dev_tp = nullptr, *dev_pi = nullptr;
    const uint8_t *dev_gv = nullptr;
};
// Results of one device search, all labels of the request in order; the request's FrontUtts point into it
struct DeviceIndex {
    std::unique_ptr<int32_t[]> pi;
    std::unique_ptr<uint8_t[]> gv;
};

const TsTables &Engine::tables() const
{
    std::lock_guard<std::mutex> lk(ts_mu);
    if (!ts) {
        ts.reset(new TsTables());
        ts_flatten(voices, std::min(voices[0]->streams.size(), (size_t)kMaxStream), ts.get());
    }
    return *ts;
}

// the caller has made `device` current
int Engine::ts_dev_for(int device, TsDev *out) const
{
    const TsTables &t = tables();
    std::lock_guard<std::mutex> lk(ts_mu);
    auto it = ts_dev.find(device);
    if (it == ts_dev.end()) {
        auto al = [](size_t b) { return (b + 15) / 16 * 16; };
        const size_t sizes[7] = {t.pool.size(),
                                 t.patterns.size() * sizeof(TsPattern),
                                 t.questions.size() * sizeof(TsQuestion),
                                 t.nodes.size() * sizeof(TsNode),
                                 t.trees.size() * sizeof(TsTree),
                                 t.models.size() * sizeof(TsModel),
                                 t.state_tree.size() * sizeof(int32_t)};
        const void *src[7] = {t.pool.data(),  t.patterns.data(), t.questions.data(),  t.nodes.data(),
                              t.trees.data(), t.models.data(),   t.state_tree.data()};
        size_t offs[7], total = 0;
        for (int k = 0; k < 7; k++) {
            offs[k] = total;
            total += al(std::max<size_t>(sizes[k], 1));
        }
        std::vector<uint8_t> host(total, 0);
        for (int k = 0; k < 7; k++)
            if (sizes[k])
                memcpy(host.data() + offs[k], src[k], sizes[k]);
        TsDevCopy c;
        hipError_t he = hipMalloc(&c.block, total);
        if (he == hipSuccess && (he = hipMemcpy(c.block, host.data(), total, hipMemcpyHostToDevice)) != hipSuccess) {
            (void)hipFree(c.block);
            c.block = nullptr;
        }
        if (he != hipSuccess)
            return hip_fail(he, "tree-search tables");
        const uint8_t *b = (const uint8_t *)c.block;
        c.d.pool = b + offs[0];
        c.d.patterns = (const TsPattern *)(b + offs[1]);
        c.d.questions = (const TsQuestion *)(b + offs[2]);
        c.d.nodes = (const TsNode *)(b + offs[3]);
        c.d.trees = (const TsTree *)(b + offs[4]);
        c.d.models = (const TsModel *)(b + offs[5]);
        c.d.state_tree = (const int32_t *)(b + offs[6]);
        c.d.nv = t.nv;
        c.d.nkind = t.nkind;
        c.d.nstate = t.nstate;
        c.d.gv_question = t.gv_question;
        c.d.memo_words = tree_search_memo_words(t.questions.size());
        it = ts_dev.emplace(device, c).first;
    }
    *out = it->second.d;
    return JB_OK;
}

// Whether the device search takes these labels: each at most kTsMaxLabel bytes, 32-bit offsets into their slab.
// *too_long (optional): the first label above the limit
static bool device_searchable(const std::vector<std::string_view> &labels, size_t *too_long = nullptr)
{
    uint64_t bytes = 0;
    for (size_t i = 0; i < labels.size(); i++) {
        if (labels[i].size() > kTsMaxLabel) {
            if (too_long)
                *too_long = i;
            return false;
        }
        bytes += labels[i].size();
    }
    if (too_long)
        *too_long = labels.size();
    return bytes < 0xffffffffull && labels.size() < 0xffffffffull;
}

// One launch for all `labels` (device_searchable) on `device` (< 0: the current one), with the tables of `te`: one
// slab up, the results back once the search's own stream has finished.  tp / pi: [n][entries], gv: [n]
static int device_tree_search(const Engine &te, int device, const std::vector<std::string_view> &labels, int32_t *tp,
                              int32_t *pi, uint8_t *gv)
{
    const size_t n = labels.size();
    if (n == 0)
        return JB_OK;
    // JB_FRONT_TRACE=1: the steps of one search on stderr (it then waits for the kernel before the read-back)
    static const bool trace = getenv("JB_FRONT_TRACE") && atoi(getenv("JB_FRONT_TRACE")) != 0;
    auto t_prev = std::chrono::steady_clock::now();
    double t_step[4] = {0, 0, 0, 0};
    auto mark = [&](int k) {
        const auto t = std::chrono::steady_clock::now();
        t_step[k] = std::chrono::duration<double, std::milli>(t - t_prev).count();
        t_prev = t;
    };
    hipError_t he;
    if (device < 0 && (he = hipGetDevice(&device)) != hipSuccess)
        return hip_fail(he, "no HIP device");
    DeviceScratch ds; // makes the device current for the call
    if ((he = ds.enter(device)) != hipSuccess)
        return hip_fail(he, "hipSetDevice");
    TsDev d;
    int rc = te.ts_dev_for(device, &d);
    if (rc)
        return rc;
    const size_t E = te.tables().entries();
    auto al = [](size_t b) { return (b + 15) / 16 * 16; };
    size_t slab_bytes = 0;
    for (const std::string_view &l : labels)
        slab_bytes += l.size();
    const size_t off_bytes = al((n + 1) * sizeof(uint32_t)), in_bytes = off_bytes + al(std::max<size_t>(slab_bytes, 1));
    const size_t idx_bytes = al(n * E * sizeof(int32_t)), out_bytes = 2 * idx_bytes + al(n);
    std::unique_ptr<uint8_t[]> in(new uint8_t[in_bytes]); // (not cleared: tens of MB for a large request)
    uint32_t *off = (uint32_t *)in.get();
    uint32_t at = 0;
    for (size_t i = 0; i < n; i++) {
        off[i] = at;
        memcpy(in.get() + off_bytes + at, labels[i].data(), labels[i].size());
        at += (uint32_t)labels[i].size();
    }
    off[n] = at;
    mark(0);
    void *blk = nullptr;
    size_t got = 0;
    if ((he = pooled_block_alloc(device, in_bytes + out_bytes, &blk, &got)) != hipSuccess)
        return hip_fail(he, "tree search: device memory");
    hipStream_t st = nullptr;
    if ((he = pooled_stream_acquire(device, &st)) != hipSuccess) {
        pooled_block_free(device, blk, got);
        return hip_fail(he, "tree search: stream");
    }
    uint8_t *b = (uint8_t *)blk;
    int32_t *tp_dev = (int32_t *)(b + in_bytes), *pi_dev = (int32_t *)(b + in_bytes + idx_bytes);
    uint8_t *gv_dev = b + in_bytes + 2 * idx_bytes;
    const char *what = "tree search: upload";
    if ((he = hipMemcpyAsync(b, in.get(), in_bytes, hipMemcpyHostToDevice, st)) == hipSuccess) {
        what = "k_tree_search";
        mark(1);
        he = launch_tree_search(d, b + off_bytes, (const uint32_t *)b, (uint32_t)n, tp ? tp_dev : nullptr, pi_dev,
                                gv_dev, st);
        if (trace && he == hipSuccess) {
            he = hipStreamSynchronize(st);
            mark(2);
        }
    }
    if (he == hipSuccess && tp) {
        what = "tree search: read-back";
        he = hipMemcpyAsync(tp, tp_dev, n * E * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    }
    if (he == hipSuccess && pi)
        he = hipMemcpyAsync(pi, pi_dev, n * E * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && gv)
        he = hipMemcpyAsync(gv, gv_dev, n, hipMemcpyDeviceToHost, st);
    const hipError_t hs = hipStreamSynchronize(st); // nothing stays in flight into the block or the host buffers
    if (he == hipSuccess && hs != hipSuccess) {
        what = "tree search";
        he = hs;
    }
    mark(3);
    pooled_stream_release(device, st);
    pooled_block_free(device, blk, got);
    if (trace)
        fprintf(stderr, "tree search on the device: %zu labels, %zu bytes; slab %.2f ms, block + upload %.2f ms, kernel "
                        "%.2f ms, read-back %.2f ms\n",
                n, slab_bytes, t_step[0], t_step[1], t_step[2], t_step[3]);
    return he == hipSuccess ? JB_OK : hip_fail(he, what);
}

// The label-line count of a request from which JB_SEARCH_AUTO searches on the device: the crossover that
// tools/front_half.py measured (profiles/r11_tree_search.txt: device mode wins front half and wall time in every shape
// from 1,024 labels on, and in none of 512 or fewer), rounded up to a power of two.
constexpr size_t kAutoSearchLines = 1024;

// Whether a request of n_lines label lines under e's mode asks for the device search
static bool wants_device_search(const Engine &e, size_t n_lines)
{
    const uint32_t mode = e.cond.tree_search;
    return n_lines > 0 && (mode == JB_SEARCH_DEVICE || (mode == JB_SEARCH_AUTO && n_lines >= kAutoSearchLines));
}

// Step 2 on the device for the utterances fu[0 .. n) of one request: one slab, one launch.  A request that holds a
// label the kernel does not take is left to the host search (nothing is counted).  count[u]: the engine utterance
// u's labels are counted for; out: what the FrontUtts then point into
static int front_search_device(const Engine &te, int device, FrontUtt *fu, size_t n, const Engine *const *count,
                               DeviceIndex *out)
{
    std::vector<std::string_view> labels;
    for (size_t u = 0; u < n; u++)
        for (const std::string &l : fu[u].pl.labels)
            labels.emplace_back(l);
    if (labels.empty() || !device_searchable(labels))
        return JB_OK;
    const size_t E = te.tables().entries();
    // (a tree's position does not depend on the label: TsTables::state_tree has it, and only the pdf indices and
    // the GV bytes come back)
    out->pi.reset(new int32_t[labels.size() * E]);
    out->gv.reset(new uint8_t[labels.size()]);
    const int rc = device_tree_search(te, device, labels, nullptr, out->pi.get(), out->gv.get());
    if (rc)
        return rc;
    size_t at = 0;
    for (size_t u = 0; u < n; u++) {
        const size_t nl = fu[u].pl.labels.size();
        fu[u].dev_tp = te.tables().state_tree.data();
        fu[u].dev_pi = out->pi.get() + at * E;
        fu[u].dev_gv = out->gv.get() + at;
        count[u]->dev_searched.fetch_add(nl, std::memory_order_relaxed);
        at += nl;
    }
    return JB_OK;
}

// Step 3.  indexed == true: the stream Gaussians are NOT blended on the host; st.iutt carries the pdf rows (tree
// search result) of every state and voice for the device-side gather: row indices into the concatenated pdf tables
// of `tables` (default e; what Engine::pdf_set_for built them for -- engines that share one voice set share the
// layout).  Labels whose trees have not been searched yet (no device block) are searched here, each on the host
// thread that finishes it.
static int front_finish(const Engine &e, FrontUtt &fu, States &st, bool indexed, unsigned label_threads,
                        const Engine *tables)
{
    const std::vector<Engine::CatTable> &cat = (tables ? tables : &e)->cat;
    const Condition &c = e.cond;
    const Voice &v0 = *e.voices[0];
    const ParsedLabels &pl = fu.pl;
    const size_t nl = pl.labels.size(), ns = (size_t)v0.meta.num_states, S = nl * ns, nv = e.voices.size();
    st.dur.assign(S, 0);
    try {
        // Models::duration (model/mod.rs:80-92) and Models::stream (:98-118) of every label in ONE parallel pass
        // (round 5: four passes, each starting and joining its own threads, were most of the front half of a
        // 200-label text -- 1.2 ms, of which the tree searches are 0.2 on six threads)
        std::vector<MV> dp(S);
        const size_t nsx = std::min(v0.streams.size(), (size_t)kMaxStream);
        const size_t nk = 1 + nsx, E = nv * nk * ns;
        size_t plen_max = 0;
        bool any_gv = false;
        for (size_t si = 0; si < nsx; si++) {
            const StreamModel &sm = v0.streams[si];
            const size_t WL = (size_t)sm.vector_length * (size_t)sm.num_windows;
            plen_max = std::max(plen_max, 2 * WL + (sm.is_msd ? 1 : 0));
            any_gv = any_gv || sm.use_gv;
            if (indexed) {
                for (size_t v = 0; v < nv; v++)
                    st.rows[si][v].assign(S, 0);
                st.weights[si] = c.w_param[si];
            } else {
                st.mean[si].assign(S * WL, 0.0);
                st.var[si].assign(S * WL, 0.0);
                st.msd[si].assign(S, DBL_MAX);
            }
        }
        const bool search_here = !fu.dev_tp;
        if (search_here) {
            fu.tp.assign(nl * E, -1);
            fu.pi.assign(nl * E, 0);
            fu.gv_on.assign(nl, 1);
        }
        const int32_t *const tp_all = search_here ? fu.tp.data() : fu.dev_tp;
        const int32_t *const pi_all = search_here ? fu.pi.data() : fu.dev_pi;
        const uint8_t *const gv_all = search_here ? fu.gv_on.data() : fu.dev_gv;
        parallel_labels(nl, label_threads, [&](size_t lo, size_t hi) {
            std::vector<double> tmp(2 * ns), buf(plen_max);
            QuestionMemo memo; // question results of the current label, per model
            for (size_t i = lo; i < hi; i++) {
                const int32_t *tp = tp_all + (search_here ? i * E : 0), *pi = pi_all + i * E;
                if (search_here) {
                    int32_t *wt = fu.tp.data() + i * E, *wp = fu.pi.data() + i * E;
                    memo.reset();
                    for (size_t v = 0; v < nv; v++) {
                        int a, b;
                        e.voices[v]->duration.get_index(2, pl.labels[i], a, b, &memo);
                        wt[v * nk * ns] = a;
                        wp[v * nk * ns] = b;
                        for (size_t si = 0; si < nsx; si++)
                            for (size_t s = 0; s < ns; s++) {
                                e.voices[v]->streams[si].stream.get_index((int)(2 + s), pl.labels[i], a, b, &memo);
                                wt[(v * nk + 1 + si) * ns + s] = a;
                                wp[(v * nk + 1 + si) * ns + s] = b;
                            }
                    }
                    if (any_gv)
                        fu.gv_on[i] = !v0.gv_off.test(pl.labels[i]);
                }
                blend(e, c.w_duration, 2 * ns, tmp.data(), [&](size_t v) {
                    return pdf_row(e.voices[v]->duration, tp[v * nk * ns], pi[v * nk * ns]);
                });
                for (size_t s = 0; s < ns; s++)
                    dp[i * ns + s] = {tmp[s], tmp[s + ns]};
                for (size_t si = 0; si < nsx; si++) {
                    const StreamModel &sm = v0.streams[si];
                    const size_t WL = (size_t)sm.vector_length * (size_t)sm.num_windows;
                    const size_t plen = 2 * WL + (sm.is_msd ? 1 : 0);
                    for (size_t s = 0; s < ns; s++) {
                        const size_t row = i * ns + s;
                        if (indexed) {
                            for (size_t v = 0; v < nv; v++) {
                                const Model &m = e.voices[v]->streams[si].stream;
                                const int t = tp[(v * nk + 1 + si) * ns + s], p = pi[(v * nk + 1 + si) * ns + s];
                                if (t < 0 || p < 1 || p > m.npdf[(size_t)t])
                                    throw ModelError("index not found"); // reference: todo!() (voice/model.rs:76-79)
                                st.rows[si][v][row] = cat[v * nsx + si].tree_off[(size_t)t] + (uint32_t)(p - 1);
                            }
                        } else {
                            blend(e, c.w_param[si], plen, buf.data(), [&](size_t v) {
                                return pdf_row(e.voices[v]->streams[si].stream, tp[(v * nk + 1 + si) * ns + s],
                                               pi[(v * nk + 1 + si) * ns + s]);
                            });
                            std::copy(buf.begin(), buf.begin() + WL, st.mean[si].begin() + row * WL);
                            std::copy(buf.begin() + WL, buf.begin() + 2 * WL, st.var[si].begin() + row * WL);
                            if (sm.is_msd)
                                st.msd[si][row] = buf[2 * WL];
                        }
                    }
                }
            }
        });
        st.dur_pdf.resize(2 * S);
        for (size_t s = 0; s < S; s++) {
            st.dur_pdf[2 * s] = dp[s].mean;
            st.dur_pdf[2 * s + 1] = dp[s].vari;
        }
        if (S) {
            if (c.phoneme_alignment) {
                // create_with_alignment (duration.rs:41-65)
                size_t frame_count = 0, next_state = 0, state = 0, nd = 0;
                for (size_t i = 0; i < nl; i++) {
                    double end_frame = pl.times[i].second;
                    if (end_frame >= 0.0) {
                        size_t cnt = state + ns - next_state;
                        estimate_with_frame_length(dp.data() + next_state, cnt,
                                                   end_frame - (double)frame_count, st.dur.data() + nd);
                        for (size_t k = 0; k < cnt; k++)
                            frame_count += st.dur[nd + k];
                        nd += cnt;
                        next_state = state + ns;
                    }
                    state += ns;
                }
                // states after the last aligned label get no duration in the reference
            } else {
                // create (duration.rs:28-38)
                estimate_duration(dp.data(), S, 0.0, st.dur.data());
                if (c.speed != 1.0) {
                    size_t length = 0;
                    for (uint32_t d : st.dur)
                        length += d;
                    estimate_with_frame_length(dp.data(), S, (double)length / c.speed, st.dur.data());
                }
            }
        }
        st.utt.num_states = (uint32_t)S;
        st.utt.durations = st.dur.data();
        // Models::stream / gv (model/mod.rs:98-146)
        for (size_t si = 0; si < v0.streams.size() && si < (size_t)kMaxStream; si++) {
            const StreamModel &sm = v0.streams[si];
            if (indexed) {
                jb_index_stream &io = st.iutt.stream[si];
                for (size_t v = 0; v < nv; v++)
                    io.row[v] = st.rows[si][v].data();
                io.weight = st.weights[si].data();
            }
            jb_stream_states &o = st.utt.stream[si];
            o.mean = st.mean[si].data();
            o.var = st.var[si].data();
            o.msd = sm.is_msd ? st.msd[si].data() : nullptr;
            o.gv_weight = c.gv_weight[si];
            o.msd_threshold = c.msd_threshold[si];
            if (sm.use_gv && nl > 0) {
                const size_t L = (size_t)sm.vector_length;
                std::vector<double> g(2 * L);
                blend(e, c.w_gv[si], 2 * L, g.data(), [&](size_t v) {
                    return e.voices[v]->streams[si].gv->get_parameter(2, pl.labels[0]); // first label only
                });
                st.gvm[si].assign(g.begin(), g.begin() + L);
                st.gvv[si].assign(g.begin() + L, g.end());
                st.gsw[si].assign(S, 0);
                for (size_t i = 0; i < nl; i++)
                    for (size_t s = 0; s < ns; s++)
                        st.gsw[si][i * ns + s] = gv_all[i];
                o.gv_mean = st.gvm[si].data();
                o.gv_var = st.gvv[si].data();
                o.gv_switch = st.gsw[si].data();
            }
            if (indexed) {
                jb_index_stream &io = st.iutt.stream[si];
                io.gv_mean = o.gv_mean;
                io.gv_var = o.gv_var;
                io.gv_switch = o.gv_switch;
                io.gv_weight = o.gv_weight;
                io.msd_threshold = o.msd_threshold;
            }
        }
        if (indexed) {
            st.iutt.num_states = (uint32_t)S;
            st.iutt.durations = st.dur.data();
            st.iutt.lf0_offset = c.additional_half_tone * kHalfTone;
        }
        // apply_additional_half_tone (stream_parameter.rs:29-37, engine.rs:342-345)
        if (!indexed && c.additional_half_tone != 0.0 && v0.streams.size() > 1) {
            const size_t WL = (size_t)v0.streams[1].vector_length * (size_t)v0.streams[1].num_windows;
            for (size_t s = 0; s < S; s++) {
                double x = st.mean[1][s * WL] + c.additional_half_tone * kHalfTone;
                st.mean[1][s * WL] = std::min(std::max(x, kMinLf0), kMaxLf0);
            }
        }
    } catch (const ModelError &ex) {
        set_error(std::string("Model error: ") + ex.what());
        return JB_ERR_MODEL;
    }
    return JB_OK;
}

// The three steps for one utterance.  search_device: -2 = host search; otherwise the device (-1: the current one)
// whose tables search the labels when e's mode asks for it
static int build_states(const Engine &e, const char *const *lines, size_t n, States &st, bool indexed = false,
                        unsigned label_threads = 1, const Engine *tables = nullptr, int search_device = -2)
{
    // JB_FRONT_TRACE=1: phases of the front half of one utterance on stderr (like JB_CREATE_TRACE / JB_REDO_TRACE)
    static const bool trace = getenv("JB_FRONT_TRACE") && atoi(getenv("JB_FRONT_TRACE")) != 0;
    auto t_prev = std::chrono::steady_clock::now();
    auto fmark = [&](const char *what) {
        if (!trace)
            return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "front half: %-28s %8.3f ms (%zu labels, %u threads)\n", what,
                std::chrono::duration<double, std::milli>(t - t_prev).count(), n, label_threads);
        t_prev = t;
    };
    FrontUtt fu;
    DeviceIndex dix;
    int rc = parse_labels(e.cond, lines, n, fu.pl);
    if (rc)
        return rc;
    fmark("labels parsed");
    if (search_device != -2 && wants_device_search(e, n)) {
        const Engine *count = &e;
        if ((rc = front_search_device(tables ? *tables : e, search_device, &fu, 1, &count, &dix)))
            return rc;
        fmark("trees searched on the device");
    }
    rc = front_finish(e, fu, st, indexed, label_threads, tables);
    fmark("pdfs, durations, GV");
    return rc;
}

// SpeechGenerator (src/speech.rs:9-96).  The reference's generator owns its three parameter tracks and a
// Vocoder and advances one frame per generate_step; nothing can change between steps, so what a step
// returns is fixed when the generator is made.  Here the whole utterance is put on the device's queue at
// creation (parameter generation, the time-chunked vocoder, the hand-off certification: the path of
// jb_synthesize) and NOT waited for; a step hands out the next frame(s) of the finished PCM from a block
// cache on the host.  Until that run has finished, the first kGenSerialFrames steps are served by the
// serial recursion one frame at a time on a side stream (persistent filter / excitation state in
// vd.state), so that the first samples arrive without waiting for the last ones.
struct Generator {
    std::unique_ptr<Batch> batch;
    size_t fperiod = 0, next = 0, total = 0;
    bool ahead_ready = false;   // the whole-utterance run is finished and certified
    bool serial_armed = false;  // the side stream waits for parameter generation
    std::vector<double> cache;  // PCM of frames [cache_first, cache_first + cache_frames)
    size_t cache_first = 0, cache_frames = 0;
    // output rate L/M of the voice's (the batch converts): step k hands out samples [ceil(k F L / M), ceil((k+1) F L / M))
    // of the converted utterance, read whole into `cache` by the first step
    uint64_t L = 1, M = 1;
    size_t out_start(size_t k) const { return (size_t)(((uint64_t)k * fperiod * L + M - 1) / M); }
    size_t out_step_max() const { return (size_t)(((uint64_t)fperiod * L + M - 1) / M); }
};
constexpr size_t kGenSerialFrames = 8;  // steps that may be served serially while the utterance is in flight
constexpr size_t kGenBlockFrames = 256; // frames per D2H block of the cache (480 KB at 240 samples per frame)

} // namespace jb

using namespace jb;

#define ENG(e) ((jb::Engine *)(e))
#define CENG(e) ((const jb::Engine *)(e))

extern "C" {

static int finish_load(std::unique_ptr<jb::Engine> &e, jb_engine **out)
{
    int rc = check_voiceset(e->voices);
    if (rc)
        return rc;
    if ((rc = load_condition(*e)))
        return rc;
    e->refresh_desc();
    *out = (jb_engine *)e.release();
    return JB_OK;
}

int jb_engine_load(const char *const *paths, size_t n, jb_engine **out)
{
    if (!out || (n && !paths))
        return JB_ERR_INVALID;
    *out = nullptr;
    std::unique_ptr<jb::Engine> e(new jb::Engine());
    try {
        for (size_t i = 0; i < n; i++)
            e->voices.push_back(load_htsvoice(paths[i]));
    } catch (const std::exception &ex) {
        set_error(std::string("Model error: ") + ex.what());
        return JB_ERR_MODEL;
    }
    return finish_load(e, out);
}

int jb_engine_load_from_bytes(const uint8_t *const *bufs, const size_t *lens, size_t n, jb_engine **out)
{
    if (!out || (n && (!bufs || !lens)))
        return JB_ERR_INVALID;
    *out = nullptr;
    std::unique_ptr<jb::Engine> e(new jb::Engine());
    try {
        for (size_t i = 0; i < n; i++)
            e->voices.push_back(parse_htsvoice(bufs[i], lens[i]));
    } catch (const std::exception &ex) {
        set_error(std::string("Model error: ") + ex.what());
        return JB_ERR_MODEL;
    }
    return finish_load(e, out);
}

// Engine::new(voices, condition) (src/engine.rs:289-291).  The reference's VoiceSet holds Arc<Voice>
// (voice_set.rs:17): the new engine SHARES the voices of `voices_of` and takes a COPY of the Condition of
// `condition_of`.  With both arguments the same engine this is Engine::clone (engine.rs:246).
int jb_engine_new(const jb_engine *voices_of, const jb_engine *condition_of, jb_engine **out)
{
    if (!out || !voices_of || !condition_of)
        return JB_ERR_INVALID;
    *out = nullptr;
    const jb::Engine *a = CENG(voices_of), *c = CENG(condition_of);
    // a Condition made for another voice set: the interpolation weights and the per-stream arrays must fit
    if (c->cond.w_duration.size() != a->voices.size() || c->cond.w_param.size() != a->voices[0]->streams.size() ||
        c->cond.msd_threshold.size() != a->voices[0]->streams.size()) {
        set_error("Weights length is invalid; the condition was made for another voice set");
        return JB_ERR_WEIGHT;
    }
    std::unique_ptr<jb::Engine> e(new jb::Engine());
    e->voices = a->voices;
    e->cond = c->cond;
    e->refresh_desc();
    *out = (jb_engine *)e.release();
    return JB_OK;
}

void jb_engine_free(jb_engine *e) { delete ENG(e); }

// ---- Condition (src/engine.rs:127-243) ----
int jb_engine_set_sampling_frequency(jb_engine *e, size_t v)
{
    ENG(e)->cond.sampling_frequency = std::max<size_t>(v, 1);
    ENG(e)->refresh_desc();
    return JB_OK;
}
size_t jb_engine_get_sampling_frequency(const jb_engine *e) { return CENG(e)->cond.sampling_frequency; }
int jb_engine_set_fperiod(jb_engine *e, size_t v)
{
    ENG(e)->cond.fperiod = std::max<size_t>(v, 1);
    ENG(e)->refresh_desc();
    return JB_OK;
}
size_t jb_engine_get_fperiod(const jb_engine *e) { return CENG(e)->cond.fperiod; }
int jb_engine_set_volume(jb_engine *e, double db)
{
    ENG(e)->cond.volume = std::exp(db * kDB);
    ENG(e)->refresh_desc();
    return JB_OK;
}
double jb_engine_get_volume(const jb_engine *e) { return std::log(CENG(e)->cond.volume) / kDB; }
int jb_engine_set_msd_threshold(jb_engine *e, size_t s, double v)
{
    if (s >= ENG(e)->cond.msd_threshold.size())
        return JB_ERR_INVALID;
    ENG(e)->cond.msd_threshold[s] = std::min(std::max(v, 0.0), 1.0);
    return JB_OK;
}
double jb_engine_get_msd_threshold(const jb_engine *e, size_t s)
{
    return s < CENG(e)->cond.msd_threshold.size() ? CENG(e)->cond.msd_threshold[s] : NAN;
}
int jb_engine_set_gv_weight(jb_engine *e, size_t s, double v)
{
    if (s >= ENG(e)->cond.gv_weight.size())
        return JB_ERR_INVALID;
    ENG(e)->cond.gv_weight[s] = std::max(v, 0.0);
    return JB_OK;
}
double jb_engine_get_gv_weight(const jb_engine *e, size_t s)
{
    return s < CENG(e)->cond.gv_weight.size() ? CENG(e)->cond.gv_weight[s] : NAN;
}
int jb_engine_set_phoneme_alignment_flag(jb_engine *e, int f)
{
    ENG(e)->cond.phoneme_alignment = f != 0;
    return JB_OK;
}
int jb_engine_get_phoneme_alignment_flag(const jb_engine *e) { return CENG(e)->cond.phoneme_alignment; }
int jb_engine_set_batch_invariant(jb_engine *e, int f)
{
    ENG(e)->cond.batch_invariant = f != 0;
    return JB_OK;
}
int jb_engine_get_batch_invariant(const jb_engine *e) { return CENG(e)->cond.batch_invariant; }
int jb_engine_set_fast_invariant(jb_engine *e, int f)
{
    ENG(e)->cond.fast_invariant = f != 0;
    return JB_OK;
}
int jb_engine_get_fast_invariant(const jb_engine *e) { return CENG(e)->cond.fast_invariant; }
int jb_engine_set_output_sampling_frequency(jb_engine *e, size_t hz)
{
    if (!e || hz > UINT32_MAX)
        return JB_ERR_INVALID;
    ENG(e)->cond.output_rate = hz;
    return JB_OK;
}
size_t jb_engine_get_output_sampling_frequency(const jb_engine *e) { return e ? CENG(e)->cond.output_rate : 0; }
int jb_engine_set_loudness_target(jb_engine *e, double lufs)
{
    if (!e)
        return JB_ERR_INVALID;
    ENG(e)->cond.loudness_target = lufs;
    return JB_OK;
}
double jb_engine_get_loudness_target(const jb_engine *e) { return e ? CENG(e)->cond.loudness_target : NAN; }
int jb_engine_set_peak_ceiling(jb_engine *e, double dbfs)
{
    if (!e)
        return JB_ERR_INVALID;
    ENG(e)->cond.peak_ceiling = dbfs;
    return JB_OK;
}
double jb_engine_get_peak_ceiling(const jb_engine *e) { return e ? CENG(e)->cond.peak_ceiling : NAN; }
int jb_engine_set_filter(jb_engine *e, const jb_filter *f)
{
    if (!e)
        return JB_ERR_INVALID;
    if (!f) {
        ENG(e)->cond.filter = jb_filter{};
        return JB_OK;
    }
    const jb::Condition &c = CENG(e)->cond;
    const size_t hz = c.output_rate ? c.output_rate : c.sampling_frequency;
    int rc = jb::filter_design_checked(f, (uint32_t)hz, 0, nullptr, "jb_engine_set_filter");
    if (rc)
        return rc;
    ENG(e)->cond.filter = *f;
    return JB_OK;
}
int jb_engine_set_fir(jb_engine *e, const jb_fir *f)
{
    if (!e)
        return JB_ERR_INVALID;
    jb::Condition &c = ENG(e)->cond;
    if (!f || (!f->taps && !f->n_taps && !f->reserved)) {
        c.fir_taps.clear();
        c.fir_hz = c.fir_delay = 0;
        return JB_OK;
    }
    const size_t hz = c.output_rate ? c.output_rate : c.sampling_frequency;
    int rc = jb::fir_check(f, (uint32_t)hz, 0, "jb_engine_set_fir");
    if (rc)
        return rc;
    c.fir_taps.assign(f->taps, f->taps + f->n_taps);
    c.fir_hz = f->hz;
    c.fir_delay = f->delay;
    c.room_on = false; // (one slot: the later call replaces the earlier)
    return JB_OK;
}
int jb_engine_set_frame_opts(jb_engine *e, const jb_frame_opts *fr)
{
    if (!e)
        return JB_ERR_INVALID;
    jb::Condition &c = ENG(e)->cond;
    if (fr)
        if (const char *f = jb::frame_opts_fault(*(const jb::FrameOpts *)fr)) {
            jb::set_error(std::string("jb_engine_set_frame_opts: ") + f);
            return JB_ERR_INVALID;
        }
    c.frame_on = fr != nullptr;
    c.frame = fr ? *fr : jb_frame_opts{};
    return JB_OK;
}
int jb_engine_set_room(jb_engine *e, const jb_room *r, uint32_t flags, uint64_t seed, double margin)
{
    if (!e)
        return JB_ERR_INVALID;
    jb::Condition &c = ENG(e)->cond;
    if (!r) {
        c.room_on = false;
        return JB_OK;
    }
    if (flags & ~JB_ROOM_VARY) {
        jb::set_error("jb_engine_set_room: flags holds an unknown flag");
        return JB_ERR_INVALID;
    }
    jb_room r0 = *r; // the room of index 0
    int rc;
    if ((flags & JB_ROOM_VARY) &&
        (rc = jb::room_vary(seed, 0, r->size, margin, r0.source, r0.mic, "jb_engine_set_room")))
        return rc;
    if ((rc = jb::room_check(&r0, 0, "jb_engine_set_room", nullptr)))
        return rc;
    const size_t hz = c.output_rate ? c.output_rate : c.sampling_frequency;
    if (r0.hz != (uint32_t)hz) {
        jb::set_error("jb_engine_set_room: hz differs from the engine's output rate (a response is never resampled): " +
                      std::to_string(r0.hz) + " Hz against " + std::to_string(hz) + " Hz");
        return JB_ERR_INVALID;
    }
    c.room_on = true;
    c.room_req = *r;
    c.room_flags = flags;
    c.room_seed = seed;
    c.room_margin = margin;
    c.fir_taps.clear(); // (one slot: the later call replaces the earlier)
    c.fir_hz = c.fir_delay = 0;
    return JB_OK;
}
int jb_engine_set_noise(jb_engine *e, const jb_noise *req)
{
    if (!e)
        return JB_ERR_INVALID;
    jb::Condition &c = ENG(e)->cond;
    if (!req) {
        c.noise_bed.clear();
        c.noise_req = jb_noise{};
        return JB_OK;
    }
    const size_t hz = c.output_rate ? c.output_rate : c.sampling_frequency;
    int rc = jb::noise_check(req, (uint32_t)hz, 0, "jb_engine_set_noise");
    if (rc)
        return rc;
    c.noise_bed.assign(req->bed, req->bed + (req->bed ? req->bed_len : 0));
    c.noise_req = *req;
    c.noise_req.bed = nullptr;
    return JB_OK;
}
int jb_engine_set_programme_mix(jb_engine *e, const jb_mix_place *place, size_t n, const jb_mix_opts *opts)
{
    if (!e)
        return JB_ERR_INVALID;
    jb::Condition &c = ENG(e)->cond;
    if (!place && n == 0) {
        c.mix_place.clear();
        c.mix_opts = jb_mix_opts{};
        return JB_OK;
    }
    if (!place || n == 0) {
        jb::set_error("jb_engine_set_programme_mix: give one place per utterance (NULL, 0 withdraws the setting)");
        return JB_ERR_INVALID;
    }
    // the request's fields through the stage's own check (the starts are set when the rate is known)
    std::vector<jb_mix_utt> req(n, jb_mix_utt{});
    std::vector<uint64_t> len(n, 0);
    for (size_t u = 0; u < n; u++) {
        if (!(place[u].start_ms >= 0.0) || !std::isfinite(place[u].start_ms)) {
            jb::set_error("jb_engine_set_programme_mix: start_ms is finite and not negative (utterance " +
                          std::to_string(u) + ")");
            return JB_ERR_INVALID;
        }
        req[u].gain_db = place[u].gain_db;
    }
    jb::MixLayout lay;
    int rc = jb::mix_layout_checked((const jb::MixUtt *)req.data(), false, len.data(), nullptr, n, sizeof(double),
                                    (const jb::MixOpts *)opts, &lay, "jb_engine_set_programme_mix");
    if (rc)
        return rc;
    c.mix_place.assign(place, place + n);
    c.mix_opts = opts ? *opts : jb_mix_opts{};
    return JB_OK;
}
int jb_engine_get_programme_mix(const jb_engine *e, jb_mix_place *place, size_t cap, size_t *n, jb_mix_opts *opts)
{
    if (!e)
        return JB_ERR_INVALID;
    const jb::Condition &c = CENG(e)->cond;
    if (n)
        *n = c.mix_place.size();
    if (opts)
        *opts = c.mix_opts;
    if (place) {
        if (cap < c.mix_place.size()) {
            jb::set_error("jb_engine_get_programme_mix: the buffer is too small");
            return JB_ERR_BUFFER;
        }
        std::copy(c.mix_place.begin(), c.mix_place.end(), place);
    }
    return JB_OK;
}
int jb_engine_get_noise(const jb_engine *e, jb_noise *out)
{
    if (!e || !out)
        return JB_ERR_INVALID;
    *out = CENG(e)->cond.noise();
    return JB_OK;
}
int jb_engine_get_filter(const jb_engine *e, jb_filter *out)
{
    if (!e || !out)
        return JB_ERR_INVALID;
    *out = CENG(e)->cond.filter;
    return JB_OK;
}
int jb_engine_set_limiter(jb_engine *e, const jb_limiter_opts *opts)
{
    if (!e)
        return JB_ERR_INVALID;
    if (!opts) {
        ENG(e)->cond.limiter_on = false;
        ENG(e)->cond.limiter = jb_limiter_opts{};
        return JB_OK;
    }
    int rc = jb::limiter_check(opts, 0, "jb_engine_set_limiter", nullptr);
    if (rc)
        return rc;
    ENG(e)->cond.limiter_on = true;
    ENG(e)->cond.limiter = *opts;
    return JB_OK;
}
int jb_engine_get_limiter(const jb_engine *e, jb_limiter_opts *out)
{
    if (!e || !out)
        return JB_ERR_INVALID;
    *out = CENG(e)->cond.limiter;
    return CENG(e)->cond.limiter_on ? 1 : 0;
}
int jb_engine_set_peak_mode(jb_engine *e, uint32_t mode)
{
    if (!e || (mode != JB_PEAK_SAMPLE && mode != JB_PEAK_TRUE))
        return JB_ERR_INVALID;
    ENG(e)->cond.peak_mode = mode;
    return JB_OK;
}
uint32_t jb_engine_get_peak_mode(const jb_engine *e) { return e ? CENG(e)->cond.peak_mode : JB_PEAK_SAMPLE; }
int jb_engine_set_loudness_scope(jb_engine *e, uint32_t scope)
{
    if (!e || (scope != JB_LOUDNESS_PER_UTTERANCE && scope != JB_LOUDNESS_PER_REQUEST))
        return JB_ERR_INVALID;
    ENG(e)->cond.loudness_scope = scope;
    return JB_OK;
}
uint32_t jb_engine_get_loudness_scope(const jb_engine *e)
{
    return e ? CENG(e)->cond.loudness_scope : JB_LOUDNESS_PER_UTTERANCE;
}
int jb_engine_set_tree_search(jb_engine *e, uint32_t mode)
{
    if (!e || (mode != JB_SEARCH_HOST && mode != JB_SEARCH_AUTO && mode != JB_SEARCH_DEVICE))
        return JB_ERR_INVALID;
    ENG(e)->cond.tree_search = mode;
    return JB_OK;
}
uint32_t jb_engine_get_tree_search(const jb_engine *e) { return e ? CENG(e)->cond.tree_search : JB_SEARCH_HOST; }
uint64_t jb_engine_device_searched_labels(const jb_engine *e)
{
    return e ? CENG(e)->dev_searched.load(std::memory_order_relaxed) : 0;
}
int jb_engine_set_speed(jb_engine *e, double v)
{
    ENG(e)->cond.speed = std::max(v, 1.0E-06);
    return JB_OK;
}
double jb_engine_get_speed(const jb_engine *e) { return CENG(e)->cond.speed; }
int jb_engine_set_alpha(jb_engine *e, double v)
{
    ENG(e)->cond.alpha = std::min(std::max(v, 0.0), 1.0);
    ENG(e)->refresh_desc();
    return JB_OK;
}
double jb_engine_get_alpha(const jb_engine *e) { return CENG(e)->cond.alpha; }
int jb_engine_set_beta(jb_engine *e, double v)
{
    ENG(e)->cond.beta = std::min(std::max(v, 0.0), 1.0);
    ENG(e)->refresh_desc();
    return JB_OK;
}
double jb_engine_get_beta(const jb_engine *e) { return CENG(e)->cond.beta; }
int jb_engine_set_additional_half_tone(jb_engine *e, double v)
{
    ENG(e)->cond.additional_half_tone = v;
    return JB_OK;
}
double jb_engine_get_additional_half_tone(const jb_engine *e) { return CENG(e)->cond.additional_half_tone; }
size_t jb_engine_num_voices(const jb_engine *e) { return CENG(e)->voices.size(); }
size_t jb_engine_num_streams(const jb_engine *e) { return (size_t)CENG(e)->voices[0]->meta.num_streams; }
size_t jb_engine_num_states(const jb_engine *e) { return (size_t)CENG(e)->voices[0]->meta.num_states; }

int jb_engine_set_interpolation_weight(jb_engine *e, int which, size_t stream, const double *w, size_t n)
{
    Condition &c = ENG(e)->cond;
    if (!w)
        return JB_ERR_INVALID;
    // Weights::new: sum must equal 1.0 within f64::EPSILON (approx default)
    double sum = 0.0;
    for (size_t i = 0; i < n; i++)
        sum += w[i];
    if (std::fabs(sum - 1.0) > DBL_EPSILON) {
        set_error("Weights do not sum to 1.0");
        return JB_ERR_WEIGHT;
    }
    if (n != ENG(e)->voices.size()) {
        set_error("Weights length is invalid; expected " + std::to_string(ENG(e)->voices.size()) +
                  ", got " + std::to_string(n));
        return JB_ERR_WEIGHT;
    }
    std::vector<double> v(w, w + n);
    if (which == 0) {
        c.w_duration = v;
    } else if (which == 1 || which == 2) {
        auto &tab = which == 1 ? c.w_param : c.w_gv;
        if (stream >= tab.size())
            return JB_ERR_INVALID; // reference: index panic
        tab[stream] = v;
    } else {
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

// InterporationWeight::{get_duration, get_parameter, get_gv} (src/model/interporation_weight.rs:115-125)
int jb_engine_get_interpolation_weight(const jb_engine *e, int which, size_t stream, double *w, size_t cap, size_t *n)
{
    const Condition &c = CENG(e)->cond;
    const std::vector<double> *v = nullptr;
    if (which == 0)
        v = &c.w_duration;
    else if (which == 1 || which == 2) {
        const auto &tab = which == 1 ? c.w_param : c.w_gv;
        if (stream >= tab.size())
            return JB_ERR_INVALID; // reference: index panic
        v = &tab[stream];
    } else {
        return JB_ERR_INVALID;
    }
    if (n)
        *n = v->size();
    if (!w)
        return JB_OK;
    if (cap < v->size())
        return JB_ERR_BUFFER;
    std::copy(v->begin(), v->end(), w);
    return JB_OK;
}

// ---- model introspection ----
static const jb::Model *model_of(const jb::Engine *e, size_t voice, int kind)
{
    if (voice >= e->voices.size())
        return nullptr;
    const Voice &v = *e->voices[voice];
    if (kind == 0)
        return &v.duration;
    if (kind >= 1 && kind <= 3 && (size_t)(kind - 1) < v.streams.size())
        return &v.streams[(size_t)(kind - 1)].stream;
    if (kind >= 4 && kind <= 6 && (size_t)(kind - 4) < v.streams.size() &&
        v.streams[(size_t)(kind - 4)].gv)
        return &*v.streams[(size_t)(kind - 4)].gv;
    return nullptr;
}

int jb_engine_model_shape(const jb_engine *e, size_t voice, int kind, size_t *ntree, size_t *pdf_len)
{
    const jb::Model *m = model_of(CENG(e), voice, kind);
    if (!m)
        return JB_ERR_INVALID;
    if (ntree)
        *ntree = m->trees.size();
    if (pdf_len)
        *pdf_len = (size_t)m->pdf_len;
    return JB_OK;
}

int jb_engine_pdf_table(const jb_engine *e, size_t voice, int kind, size_t tree, const float **table,
                        size_t *npdf)
{
    const jb::Model *m = model_of(CENG(e), voice, kind);
    if (!m || tree >= m->trees.size() || !table)
        return JB_ERR_INVALID;
    *table = m->pdf[tree].data();
    if (npdf)
        *npdf = (size_t)m->npdf[tree];
    return JB_OK;
}

int jb_engine_tree_index(const jb_engine *e, size_t voice, int kind, int state_index, const char *label,
                         int *tree_state, int *pdf_index)
{
    const jb::Model *m = model_of(CENG(e), voice, kind);
    if (!m || !label)
        return JB_ERR_INVALID;
    int tp, pi;
    m->get_index(state_index, label, tp, pi);
    if (tree_state)
        *tree_state = tp < 0 ? -1 : m->trees[(size_t)tp].state;
    if (pdf_index)
        *pdf_index = pi;
    return JB_OK;
}

// tree positions of a search -> the trees' states, as jb_engine_tree_index reports them
static void positions_to_states(const jb::TsTables &t, size_t n_labels, int32_t *tree_state)
{
    const size_t E = t.entries();
    for (size_t i = 0; i < n_labels; i++)
        for (size_t k = 0; k < E; k++) {
            int32_t &v = tree_state[i * E + k];
            if (v >= 0)
                v = t.trees[t.models[k / t.nstate].tree0 + (uint32_t)v].state;
        }
}

int jb_tree_search_flat_host(const jb_engine *e, const char *const *labels, size_t n_labels, int32_t *tree_state,
                             int32_t *pdf_index, uint8_t *gv_on)
{
    if (!e || (n_labels && !labels))
        return JB_ERR_INVALID;
    for (size_t i = 0; i < n_labels; i++)
        if (!labels[i])
            return JB_ERR_INVALID;
    const jb::TsTables &t = CENG(e)->tables();
    const size_t E = t.entries();
    std::vector<int32_t> tp(E), pi(E);
    std::vector<int8_t> memo;
    for (size_t i = 0; i < n_labels; i++) {
        uint8_t g = 0;
        jb::ts_walk_label(t, labels[i], tp.data(), pi.data(), &g, memo);
        if (tree_state)
            std::copy(tp.begin(), tp.end(), tree_state + i * E);
        if (pdf_index)
            std::copy(pi.begin(), pi.end(), pdf_index + i * E);
        if (gv_on)
            gv_on[i] = g;
    }
    if (tree_state)
        positions_to_states(t, n_labels, tree_state);
    return JB_OK;
}

int jb_tree_search_batch(const jb_engine *e, const char *const *labels, size_t n_labels, int32_t device,
                         int32_t *tree_state, int32_t *pdf_index, uint8_t *gv_on)
{
    if (!e || (n_labels && !labels))
        return JB_ERR_INVALID;
    std::vector<std::string_view> views(n_labels);
    for (size_t i = 0; i < n_labels; i++) {
        if (!labels[i])
            return JB_ERR_INVALID;
        views[i] = labels[i];
    }
    size_t bad = 0;
    if (!device_searchable(views, &bad)) {
        set_error(bad < n_labels ? "jb_tree_search_batch: labels[" + std::to_string(bad) + "] has " +
                                       std::to_string(views[bad].size()) + " bytes; the device search takes at most " +
                                       std::to_string(jb::kTsMaxLabel)
                                 : std::string("jb_tree_search_batch: the labels exceed 4 GiB"));
        return JB_ERR_UNSUPPORTED;
    }
    const int rc = device_tree_search(*CENG(e), device, views, tree_state, pdf_index, gv_on);
    if (!rc && tree_state)
        positions_to_states(CENG(e)->tables(), n_labels, tree_state);
    return rc;
}

// ---- states ----
int jb_engine_states(const jb_engine *e, const char *const *lines, size_t n, jb_states **out)
{
    if (!e || !out || (n && !lines))
        return JB_ERR_INVALID;
    *out = nullptr;
    std::unique_ptr<jb::States> st(new jb::States());
    int rc = build_states(*CENG(e), lines, n, *st, false, host_threads_default(), nullptr, -1);
    if (rc)
        return rc;
    *out = (jb_states *)st.release();
    return JB_OK;
}
const jb_state_utt *jb_states_utt(const jb_states *s) { return s ? &((const jb::States *)s)->utt : nullptr; }
const double *jb_states_duration_params(const jb_states *s)
{
    return s && !((const jb::States *)s)->dur_pdf.empty() ? ((const jb::States *)s)->dur_pdf.data() : nullptr;
}
const jb_voice_desc *jb_engine_voice_desc(const jb_engine *e) { return e ? &CENG(e)->desc : nullptr; }
void jb_states_free(jb_states *s) { delete (jb::States *)s; }

// ---- synthesize ----
void jb_pcm_free(double *p) { free(p); }

// ---- WAV sink (examples/is-bonsai/main.rs:37-49) ----
static int write_wav(const char *path, const int16_t *pcm, size_t n, uint32_t fs)
{
    if (!path || (!pcm && n) || n > (0xffffffffull - 36) / 2) {
        jb::set_error("bad WAV arguments");
        return JB_ERR_INVALID;
    }
    FILE *f = fopen(path, "wb");
    if (!f) {
        jb::set_error(std::string("cannot open ") + path + ": " + strerror(errno));
        return JB_ERR_MODEL;
    }
    const uint32_t data = (uint32_t)(n * 2), riff = 36 + data, fmt_len = 16, byte_rate = fs * 2;
    const uint16_t pcm_tag = 1, ch = 1, align = 2, bits = 16;
    bool ok = fwrite("RIFF", 1, 4, f) == 4 && fwrite(&riff, 4, 1, f) == 1 && fwrite("WAVEfmt ", 1, 8, f) == 8 &&
              fwrite(&fmt_len, 4, 1, f) == 1 && fwrite(&pcm_tag, 2, 1, f) == 1 && fwrite(&ch, 2, 1, f) == 1 &&
              fwrite(&fs, 4, 1, f) == 1 && fwrite(&byte_rate, 4, 1, f) == 1 && fwrite(&align, 2, 1, f) == 1 &&
              fwrite(&bits, 2, 1, f) == 1 && fwrite("data", 1, 4, f) == 4 && fwrite(&data, 4, 1, f) == 1 &&
              (n == 0 || fwrite(pcm, 2, n, f) == n); // little-endian host (x86-64)
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        jb::set_error(std::string("short write to ") + path);
        return JB_ERR_MODEL;
    }
    return JB_OK;
}

int jb_write_wav_i16(const char *path, const int16_t *pcm, size_t n, uint32_t fs) { return write_wav(path, pcm, n, fs); }

int jb_write_wav_f64(const char *path, const double *pcm, size_t n, uint32_t fs)
{
    if (!pcm && n)
        return JB_ERR_INVALID;
    std::vector<int16_t> q(n);
    for (size_t i = 0; i < n; i++) {
        double v = std::fmin(pcm[i], 32767.0);
        v = std::fmax(v, -32768.0);
        q[i] = (int16_t)(int)v; // `as i16`: truncation toward zero
    }
    return write_wav(path, q.data(), n, fs);
}

} // extern "C"

namespace {

typedef std::chrono::steady_clock::time_point TimePoint;
TimePoint now() { return std::chrono::steady_clock::now(); }
double ms(TimePoint a, TimePoint b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// fn(u) for every u of [lo, hi) on up to nt host threads; the first failure in utterance order, with its message
template <class F> int each_utt(size_t lo, size_t hi, unsigned nt, F fn)
{
    std::vector<int> rcs(hi - lo, JB_OK);
    std::vector<std::string> errs(hi - lo);
    std::atomic<size_t> next{lo};
    auto work = [&]() {
        for (size_t u; (u = next.fetch_add(1)) < hi;) {
            rcs[u - lo] = fn(u);
            if (rcs[u - lo])
                errs[u - lo] = jb::g_err; // the worker's thread-local message
        }
    };
    const unsigned n = (unsigned)std::min<size_t>(nt, hi - lo);
    if (n <= 1) {
        work();
    } else {
        std::vector<std::thread> pool;
        for (unsigned k = 0; k < n; k++)
            pool.emplace_back(work);
        for (auto &t : pool)
            t.join();
    }
    for (size_t u = lo; u < hi; u++)
        if (rcs[u - lo]) {
            jb::set_error(errs[u - lo]);
            return rcs[u - lo];
        }
    return JB_OK;
}

// One engine request on its way through: the state its steps share
struct SynthRun {
    const jb::SynthRequest &rq;
    const size_t elem;  // bytes per PCM sample of the batches: 8 (f64, Engine::synthesize's Vec<f64>) or 2 (the fused
                        // 16-bit sink)
    // JB_E2E_TIMING=1: time spent in the four phases on stderr (tools/e2e_engine.py); with more than
    // one group they overlap, so their sum exceeds the wall time
    const bool timing;
    unsigned nt = 1;    // host threads of the front half
    int32_t device;
    // the engine's pdf tables on the device: the batches are made from pdf rows, not from blended states (null:
    // JB_HOST_BLEND)
    const jb_pdf_set *pset = nullptr;
    bool one_gain = false;            // per-request loudness scope: one loudness group
    std::vector<std::unique_ptr<jb::States>> sts; // [n_utts]
    std::vector<size_t> glo;                      // [ngroups + 1] plan_synth_groups
    std::vector<std::unique_ptr<jb::Batch>> batches; // [ngroups]
    double t_front = 0, t_create = 0, t_wait = 0, t_d2h = 0;

    explicit SynthRun(const jb::SynthRequest &r)
        : rq(r), elem(r.i16 ? sizeof(int16_t) : sizeof(double)),
          timing(getenv("JB_E2E_TIMING") && atoi(getenv("JB_E2E_TIMING")) != 0), device(r.device)
    {
    }
    size_t ngroups() const { return glo.size() - 1; }
    const jb::Engine *eng(size_t u) const { return CENG(rq.each ? rq.each[u] : rq.e); } // the engine of utterance u

    int resolve_device();
    int front_half(size_t lo, size_t hi);
    int create_batch(size_t g);
    int apply_conditions(jb::OutputChain &out, size_t lo, size_t hi);
    int request_programme(jb::OutputChain &out, size_t lo, size_t hi);
    int read_stem_reports(jb::Batch *b);
    int launch(size_t g);
    int wait_group(size_t g);
    int read_group(size_t g);
    int read_outputs(jb::Batch *b, size_t lo, size_t hi);
    int finish(size_t g)
    {
        const int rc = wait_group(g);
        return rc ? rc : read_group(g);
    }
    int run_pipelined();
};

// The host threads of the front half, and the device and pdf set of the request
int SynthRun::resolve_device()
{
    // The front half (label parse, tree search, pdf blend, durations: label.rs, model/mod.rs:80-156,
    // duration.rs) is independent per utterance and read-only on the engine: host threads, one
    // utterance at a time each (JB_HOST_THREADS, default min(16, cores)).  It is ~13 ms per 128 s
    // utterance and thread against ~0.7 ms of GPU time.
    nt = host_threads_default();
    if (rq.host_threads && !getenv("JB_HOST_THREADS")) // a multi-device call shares the host cores between its device threads
        nt = rq.host_threads;
    // device-side gather + blend unless JB_HOST_BLEND=1 (A/B: both produce the same bits)
    const bool host_blend = getenv("JB_HOST_BLEND") && atoi(getenv("JB_HOST_BLEND")) != 0;
    if (!host_blend) {
        int dev = device;
        if (dev < 0 && hipGetDevice(&dev) != hipSuccess) {
            jb::set_error("no HIP device");
            return JB_ERR_DEVICE;
        }
        int prc = CENG(rq.e)->pdf_set_for(dev, &pset);
        if (prc)
            return prc;
        device = dev;
    }
    return JB_OK;
}

// The front half of the utterances [lo, hi) on the host threads: labels to states (sts[u])
int SynthRun::front_half(size_t lo, size_t hi)
{
    const auto t0 = now();
    const jb::Engine &e = *CENG(rq.e);
    const char *const *lines = rq.lines;
    const size_t *line_off = rq.line_off;
    const bool indexed = pset != nullptr;
    // fewer utterances than threads (a single long text through jb_synthesize): the spare threads split
    // each utterance's labels
    const unsigned per_utt = (unsigned)std::max<size_t>(1, nt / std::max<size_t>(1, hi - lo));
    int rc;
    if (wants_device_search(e, line_off[hi] - line_off[lo])) {
        // the group's labels through one launch: parse on the host threads, one slab up, the indices back,
        // finish on the host threads
        std::vector<jb::FrontUtt> fu(hi - lo);
        jb::DeviceIndex dix;
        std::vector<const jb::Engine *> count(hi - lo);
        for (size_t u = lo; u < hi; u++)
            count[u - lo] = eng(u);
        rc = each_utt(lo, hi, nt, [&](size_t u) {
            return parse_labels(eng(u)->cond, lines + line_off[u], line_off[u + 1] - line_off[u], fu[u - lo].pl);
        });
        const auto t1 = now();
        if (!rc)
            rc = front_search_device(e, device, fu.data(), fu.size(), count.data(), &dix);
        const auto t2 = now();
        if (!rc)
            rc = each_utt(lo, hi, nt,
                          [&](size_t u) { return front_finish(*eng(u), fu[u - lo], *sts[u], indexed, per_utt, &e); });
        if (timing)
            fprintf(stderr, "front half of %zu utterance(s): parse %.2f ms, device search %.2f ms, finish %.2f ms\n",
                    hi - lo, ms(t0, t1), ms(t1, t2), ms(t2, now()));
    } else {
        rc = each_utt(lo, hi, nt, [&](size_t u) {
            return build_states(*eng(u), lines + line_off[u], line_off[u + 1] - line_off[u], *sts[u], indexed, per_utt,
                                &e);
        });
    }
    t_front += ms(t0, now());
    return rc;
}

// The batch of group g (batches[g]) from its utterances' states: indexed or state-level
int SynthRun::create_batch(size_t g)
{
    const size_t lo = glo[g], hi = glo[g + 1];
    const jb::Engine &e = *CENG(rq.e);
    jb_batch_opts opts{};
    opts.device = device;
    opts.flags = (elem == 2 ? JB_BATCH_PCM_I16 : 0) | e.cond.batch_flags();
    jb::Batch *b = nullptr;
    int rc;
    // one engine per utterance: the vocoder conditions of the utterances (a batch whose entries are all the
    // same runs as one made without them)
    std::vector<jb_utt_voc> voc(rq.each ? hi - lo : 0);
    for (size_t u = lo; rq.each && u < hi; u++)
        voc[u - lo] = jb_utt_voc{eng(u)->cond.alpha, eng(u)->cond.beta, eng(u)->cond.volume};
    const jb_utt_voc *vp = rq.each ? voc.data() : nullptr;
    if (pset) {
        std::vector<jb_index_utt> iu(hi - lo);
        for (size_t u = lo; u < hi; u++)
            iu[u - lo] = sts[u]->iutt;
        rc = jb_batch_create_indexed_voc(&e.desc, pset, iu.data(), hi - lo, vp, &opts, (jb_batch **)&b);
    } else {
        std::vector<jb_state_utt> su(hi - lo);
        for (size_t u = lo; u < hi; u++)
            su[u - lo] = sts[u]->utt;
        rc = jb::Batch::create(&e.desc, su.data(), hi - lo, &opts, &b, nullptr, nullptr, vp);
    }
    if (!rc)
        batches[g].reset(b);
    return rc;
}

// The output conditions of the utterances [lo, hi), each its engine's own: rate, filter, loudness, peak mode, limiter; then the
// request's one loudness group and its encoder (the setters' refusals depend on this order)
int SynthRun::apply_conditions(jb::OutputChain &out, size_t lo, size_t hi)
{
    int rc;
    // output rate: each utterance's engine's own (a batch whose utterances are all native converts nothing)
    std::vector<uint32_t> rates(hi - lo);
    bool any_rate = false;
    for (size_t u = lo; u < hi; u++) {
        rates[u - lo] = (uint32_t)eng(u)->cond.output_rate;
        any_rate = any_rate || rates[u - lo];
    }
    if (any_rate && (rc = out.set_output_rate(rates.data(), rates.size())))
        return rc;
    // the filter: each utterance's engine's own (a batch whose engines all have none filters nothing)
    std::vector<jb_filter> filters(hi - lo);
    bool any_filter = false;
    for (size_t u = lo; u < hi; u++) {
        filters[u - lo] = eng(u)->cond.filter;
        any_filter = any_filter || filters[u - lo].n_sections;
    }
    if (any_filter && (rc = out.set_filter(filters.data(), filters.size())))
        return rc;
    // the impulse response: each utterance's engine's own, the same way
    std::vector<jb_fir> firs(hi - lo);
    bool any_fir = false;
    for (size_t u = lo; u < hi; u++) {
        firs[u - lo] = eng(u)->cond.fir();
        any_fir = any_fir || firs[u - lo].taps;
    }
    // the room: each utterance's engine's own, in the response's slot; JB_ROOM_VARY varies the positions by the
    // utterance's index in the call
    std::vector<jb_room> rooms(hi - lo);
    bool any_room = false;
    for (size_t u = lo; u < hi; u++) {
        if ((rc = eng(u)->cond.room(u, &rooms[u - lo])))
            return rc;
        any_room = any_room || eng(u)->cond.room_on;
    }
    if (any_room ? (rc = out.set_room(rooms.data(), rooms.size(), firs.data()))
                 : (any_fir && (rc = out.set_fir(firs.data(), firs.size()))))
        return rc;
    // the noise: each utterance's engine's own; JB_NOISE_VARY varies by the utterance's index in the call
    std::vector<jb_noise> noises(hi - lo);
    std::vector<uint64_t> call_k(hi - lo);
    bool any_noise = false;
    for (size_t u = lo; u < hi; u++) {
        noises[u - lo] = eng(u)->cond.noise();
        call_k[u - lo] = u;
        any_noise = any_noise || noises[u - lo].bed || noises[u - lo].kind != JB_NOISE_BED;
    }
    if (any_noise && (rc = out.set_noise(noises.data(), noises.size(), call_k.data())))
        return rc;
    // loudness: each utterance's engine's own target and ceiling; an engine without a target leaves its
    // utterance as it is (measured, gain 0 dB: bit for bit the same) when another engine of the batch has one
    std::vector<double> targets(hi - lo), ceilings(hi - lo);
    std::vector<uint32_t> modes(hi - lo);
    bool any_target = false, any_true = false;
    for (size_t u = lo; u < hi; u++) {
        const bool on = !std::isnan(eng(u)->cond.loudness_target);
        targets[u - lo] = on ? eng(u)->cond.loudness_target : NAN;
        ceilings[u - lo] = on ? eng(u)->cond.peak_ceiling : INFINITY;
        modes[u - lo] = on ? eng(u)->cond.peak_mode : JB_PEAK_SAMPLE;
        any_target = any_target || on;
        any_true = any_true || modes[u - lo] == JB_PEAK_TRUE;
    }
    if (any_target && (rc = out.set_loudness(targets.data(), ceilings.data(), targets.size())))
        return rc;
    if (any_true && (rc = out.set_peak_mode(modes.data(), modes.size())))
        return rc;
    // the limiter: each utterance's engine's own (an engine without one leaves its utterance to the plain apply pass;
    // inside the request's one group the setters refuse engines that disagree)
    std::vector<jb_limiter_opts> limiters(hi - lo);
    bool any_limiter = false;
    for (size_t u = lo; u < hi; u++) {
        const bool on = eng(u)->cond.limiter_on && !std::isnan(eng(u)->cond.loudness_target);
        limiters[u - lo] = on ? eng(u)->cond.limiter : jb_limiter_opts{0.0, 0.0, 0.0, JB_LIMITER_OFF, 0};
        any_limiter = any_limiter || on;
    }
    if (any_limiter && (rc = out.set_limiter(limiters.data(), limiters.size())))
        return rc;
    if (one_gain) {
        const std::vector<uint32_t> group(hi - lo, 0u);
        if ((rc = out.set_loudness_groups(group.data(), group.size())))
            return rc;
    }
    // the request's encoder
    if (rq.sink == jb::SynthSink::Flac &&
        ((rc = out.set_flac(rq.flac)) || (rq.flac_meta && (rc = out.set_flac_meta(rq.flac_meta)))))
        return rc;
    if (rq.sink == jb::SynthSink::Formatted && (rc = out.set_format(rq.fmt)))
        return rc;
    if (rq.sink == jb::SynthSink::Adpcm && (rc = out.set_adpcm(rq.adpcm)))
        return rc;
    // the frame request beside the two feature encoders: the engines' own, which must agree (one per batch)
    if (rq.sink == jb::SynthSink::Fbank || rq.sink == jb::SynthSink::Mfcc) {
        const jb::Condition &c0 = eng(lo)->cond;
        for (size_t u = lo; u < hi; u++)
            if (eng(u)->cond.frame_on != c0.frame_on || memcmp(&eng(u)->cond.frame, &c0.frame, sizeof c0.frame)) {
                jb::set_error("jb_engine_set_frame_opts: the engines of one call must agree on the frame request");
                return JB_ERR_INVALID;
            }
        if (c0.frame_on && (rc = out.set_frame_opts(&c0.frame)))
            return rc;
    }
    if (rq.sink == jb::SynthSink::Fbank && (rc = out.set_fbank(rq.fbank)))
        return rc;
    if (rq.sink == jb::SynthSink::Mfcc && (rc = out.set_mfcc(rq.fbank, rq.mfcc)))
        return rc;
    if (rq.sink == jb::SynthSink::Melspec && (rc = out.set_melspec(rq.melspec)))
        return rc;
    if (rq.sink == jb::SynthSink::Pitch && (rc = out.set_pitch(rq.pitch)))
        return rc;
    return JB_OK;
}

// The utterances [lo, hi) of the batch as one programme, and each member's start to the caller
int SynthRun::request_programme(jb::OutputChain &out, size_t lo, size_t hi)
{
    const jb_join_opts *join = rq.join;
    // One programme, every member under the fade at both its edges, in samples at the output rate.  A join: the lead in
    // front of the first member, the gap behind every member but the last, the trail behind the last.  With
    // jb_engine_set_programme_mix a mix: member u starts at lead + start_ms[u] under its gain, and the trail is every
    // member's pad behind it (the entry has checked count and gap)
    const Condition &c0 = eng(lo)->cond;
    const bool mix = !c0.mix_place.empty();
    const uint32_t hz = out.utt(0).hz;
    const size_t n = hi - lo;
    const uint32_t fade = (uint32_t)std::min<uint64_t>(jb::join_ms_to_samples(join->fade_ms, hz), 0xffffffffu);
    // one request, in the words of its kind: the two differ in where a member's place and its gain come from
    std::vector<jb_join_utt> jreq(mix ? 0 : n, jb_join_utt{});
    std::vector<jb_mix_utt> mreq(mix ? n : 0, jb_mix_utt{});
    for (size_t u = 0; u < n; u++) {
        if (mix) {
            mreq[u].fade_in = mreq[u].fade_out = fade;
            mreq[u].start = jb::join_ms_to_samples(join->lead_ms + c0.mix_place[u].start_ms, hz);
            mreq[u].pad_after = jb::join_ms_to_samples(join->trail_ms, hz);
            mreq[u].gain_db = c0.mix_place[u].gain_db;
        } else {
            jreq[u].fade_in = jreq[u].fade_out = fade;
            jreq[u].pad_before = u == 0 ? jb::join_ms_to_samples(join->lead_ms, hz) : 0;
            jreq[u].pad_after = jb::join_ms_to_samples(u + 1 == n ? join->trail_ms : join->gap_ms, hz);
        }
    }
    int rc = mix ? out.set_mix(mreq.data(), n, &c0.mix_opts) : out.set_join(jreq.data(), n);
    if (!rc && rq.stem_of) // (the entry has checked that the engine holds a mix)
        rc = out.set_mix_stems(rq.stem_of + lo, n, rq.stem_flags);
    if (rc)
        return rc;
    for (size_t u = 0; rq.join_starts && u < n; u++)
        rq.join_starts[lo + u] = out.member_start(u);
    return JB_OK;
}

// Group g onto the device: its batch, the requests to its output chain, and the run (not waited for)
int SynthRun::launch(size_t g)
{
    const auto t0 = now();
    const size_t lo = glo[g], hi = glo[g + 1];
    int rc = create_batch(g);
    if (rc)
        return rc;
    jb::Batch *b = batches[g].get();
    if ((rc = apply_conditions(b->out, lo, hi)) || (rq.join && (rc = request_programme(b->out, lo, hi))) ||
        (rq.activity && (rc = b->out.set_activity(rq.activity))))
        return rc;
    rc = b->run(false);
    t_create += ms(t0, now());
    return rc;
}

// Until the device has finished group g
int SynthRun::wait_group(size_t g)
{
    const auto t0 = now();
    const int rc = batches[g]->sync();
    t_wait += ms(t0, now());
    return rc;
}

// The outputs of group g into buffers of the caller's (malloc), and its batch back to the pools
int SynthRun::read_group(size_t g)
{
    const auto t0 = now();
    const int rc = read_outputs(batches[g].get(), glo[g], glo[g + 1]);
    batches[g].reset(); // device memory and streams back to the pools
    t_d2h += ms(t0, now());
    return rc;
}

// With a stems request: the number of outputs and each stem's report to the caller
int SynthRun::read_stem_reports(jb::Batch *b)
{
    if (!rq.stem_of)
        return JB_OK;
    const size_t U = b->out.num_outputs(), P = b->out.num_programmes();
    for (size_t p = P; rq.stem_reports && p < U; p++) {
        const int rc = b->out.read_stem(p, rq.stem_reports + (p - P));
        if (rc)
            return rc;
    }
    if (rq.n_outputs) // (last: a call that fails hands out nothing and says so)
        *rq.n_outputs = U;
    return JB_OK;
}

// read_group: what the request's sink and join hand out for the utterances [lo, hi) of batch b
int SynthRun::read_outputs(jb::Batch *b, size_t lo, size_t hi)
{
    void **pcm = rq.out;
    size_t *n_samples = rq.n_out;
    if (rq.sink != jb::SynthSink::Pcm) {
        // the used bytes of the sink's slab in one copy (FLAC: behind the streams' sizes and places, one small copy),
        // then each output's share
        std::vector<jb::ByteSpan> places;
        std::unique_ptr<uint8_t[]> host;
        int rc = b->out.read_bytes_all(rq.sink, &places, &host);
        std::vector<jb::PcmShare> shares;
        for (const jb::ByteSpan &w : places)
            shares.push_back({w.off, w.bytes});
        if (rc || (rc = jb::hand_out(host.get(), 1, shares, pcm + lo, n_samples + lo)))
            return rc;
        // the request's count of each output: the samples its ADPCM blocks encode, or its frames of features
        for (size_t p = 0; rq.counts && p < places.size(); p++)
            rq.counts[lo + p] = rq.sink == jb::SynthSink::Fbank  ? (size_t)b->out.fbank_place(p).T
                                : rq.sink == jb::SynthSink::Mfcc ? (size_t)b->out.mfcc_place(p).T
                                : rq.sink == jb::SynthSink::Melspec ? (size_t)b->out.melspec_place(p).T
                                : rq.sink == jb::SynthSink::Pitch ? (size_t)b->out.pitch_place(p).T
                                : rq.join                        ? (size_t)b->out.programme(p).n
                                                                 : b->out.samples(p);
        return read_stem_reports(b);
    }
    if (rq.join && rq.stem_of) {
        // the mixture and the stems behind it, unit after unit
        for (size_t p = 0; p < b->out.num_outputs(); p++) {
            const size_t ns = (size_t)b->out.programme(p).n;
            if (!(pcm[p] = malloc(std::max<size_t>(ns, 1) * elem))) {
                jb::set_error("out of host memory");
                return JB_ERR_INVALID;
            }
            n_samples[p] = ns;
            const int rc = b->out.read_programme(p, elem == 2, pcm[p]);
            if (rc)
                return rc;
        }
        return read_stem_reports(b);
    }
    if (rq.join) {
        // the programme's PCM in one copy
        const size_t ns = (size_t)b->out.programme(0).n;
        if (!(pcm[0] = malloc(std::max<size_t>(ns, 1) * elem))) {
            jb::set_error("out of host memory");
            return JB_ERR_INVALID;
        }
        n_samples[0] = ns;
        int rc = b->out.read_programme(0, elem == 2, pcm[0]);
        if (rc || !rq.activity)
            return rc;
        // the programme's labels beside it
        jb::ActLayUnit w{};
        if ((rc = b->out.activity_place(0, true, "jb_synthesize_programme_activity", &w)))
            return rc;
        if (!(rq.act_out[0] = (uint8_t *)malloc(std::max<size_t>((size_t)(w.T * w.C), 1)))) {
            jb::set_error("out of host memory");
            return JB_ERR_INVALID;
        }
        rq.act_T[0] = w.T;
        rq.act_C[0] = w.C;
        return b->out.read_activity(0, rq.act_out[0]);
    }
    for (size_t u = lo; u < hi; u++) {
        const size_t ns = b->out.samples(u - lo);
        n_samples[u] = ns;
        if (!ns)
            continue;
        // 2 MB alignment + MADV_HUGEPAGE: where transparent huge pages are allowed, the first touch of
        // the buffer (by the scatter threads) takes 512x fewer faults; free() releases it as usual
        const size_t bytes = ns * elem;
        if (bytes >= (4u << 20) && posix_memalign(&pcm[u], 2u << 20, bytes) == 0)
            madvise(pcm[u], bytes, MADV_HUGEPAGE);
        else
            pcm[u] = malloc(bytes);
        if (!pcm[u]) {
            jb::set_error("out of host memory");
            return JB_ERR_INVALID;
        }
    }
    // whole slab through the pinned staging ring into the per-utterance buffers
    return b->read_pcm_split(pcm + lo, elem);
}

// More than one group: the main thread runs front half and launch of group after group, a finisher thread waits for
// and reads them
int SynthRun::run_pipelined()
{
    // f64 in groups (JB_SYNTH_GROUPS only): all groups' GPU work first, then the read-backs, so that no
    // read-back runs beside kernels
    const bool d2h_last = elem == 8 && rq.sink != jb::SynthSink::Formatted;
    // finisher thread: groups in order, as soon as they are launched
    std::mutex mu;
    std::condition_variable cv;
    size_t launched = 0;
    bool stop = false;
    int frc = JB_OK;
    std::string ferr;
    auto failed = [&](int r) {
        if (r) {
            std::lock_guard<std::mutex> lk(mu);
            frc = r;
            ferr = jb::g_err;
        }
        return r != 0;
    };
    std::thread finisher([&]() {
        for (size_t g = 0; g < ngroups(); g++) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return launched > g || stop; });
                if (launched <= g)
                    return;
            }
            if (failed(d2h_last ? wait_group(g) : finish(g)))
                return;
        }
        for (size_t g = 0; d2h_last && g < ngroups(); g++)
            if (failed(read_group(g)))
                return;
    });
    int rc = JB_OK;
    for (size_t g = 0; g < ngroups() && !rc; g++) {
        if ((rc = front_half(glo[g], glo[g + 1])) || (rc = launch(g)))
            break;
        std::lock_guard<std::mutex> lk(mu);
        launched = g + 1;
        cv.notify_all();
        if (frc)
            break;
    }
    {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
        cv.notify_all();
    }
    finisher.join();
    if (!rc && frc) {
        rc = frc;
        jb::set_error(ferr);
    }
    return rc;
}

} // namespace

int jb::synthesize_batch_impl(const SynthRequest &rq)
{
    if (!rq.e || !rq.out || !rq.n_out || (rq.n_utts && !rq.line_off))
        return JB_ERR_INVALID;
    // with a join the call hands out ONE output, the programme of all its utterances
    // (with a stems request the mixture and at most one stem per utterance behind it)
    const size_t n_outs = rq.join ? (rq.stem_of ? 1 + rq.n_utts : 1) : rq.n_utts;
    if (rq.n_outputs)
        *rq.n_outputs = 0;
    for (size_t u = 0; u < n_outs; u++) {
        rq.out[u] = nullptr;
        rq.n_out[u] = 0;
    }
    SynthRun run(rq);
    run.sts.resize(rq.n_utts);
    for (auto &st : run.sts)
        st.reset(new jb::States());
    const auto t_start = now();
    int rc = run.resolve_device();
    if (rc)
        return rc;

    // A large request goes through in two groups: while the GPU works on the first, the host threads
    // run the front half of the second.  With the 16-bit sink the read-back of the first group also
    // runs beside the GPU work of the second (134 -> 113 ms for 64 x 157 s); with f64 PCM a read-back
    // beside running kernels slows down by more than the overlap gains (203 -> 242 ms), so there all
    // GPU work comes first and the read-backs after it (203-224 -> 183 ms).  More groups lose (three:
    // 220 ms): smaller batches fill the chip less well and their blocks miss the pool.
    // Groups split the utterances by label count; JB_SYNTH_GROUPS overrides.
    const char *ev = getenv("JB_SYNTH_GROUPS");
    // per-request loudness scope: the request is one loudness group, and a group lives in one batch
    run.one_gain = CENG(rq.e)->cond.loudness_scope == JB_LOUDNESS_PER_REQUEST &&
                   !std::isnan(CENG(rq.e)->cond.loudness_target);
    // (a programme lives in one batch too)
    run.glo = plan_synth_groups(rq.line_off, rq.n_utts, ev ? std::max(1, atoi(ev)) : 0, run.one_gain || rq.join);
    run.batches.resize(run.ngroups());

    if (run.ngroups() == 1) {
        if (!(rc = run.front_half(0, rq.n_utts)) && !(rc = run.launch(0)))
            rc = run.finish(0);
    } else {
        rc = run.run_pipelined();
    }
    if (rc) {
        run.batches.clear();
        if (rq.n_outputs)
            *rq.n_outputs = 0;
        for (size_t u = 0; u < n_outs; u++) {
            free(rq.out[u]);
            rq.out[u] = nullptr;
            rq.n_out[u] = 0;
        }
        return rc;
    }
    if (run.timing)
        fprintf(stderr,
                "jb_synthesize_batch: %zu group(s), wall %.1f ms; front half %.1f ms, upload+create+enqueue %.1f ms, "
                "wait for the GPU %.1f ms, D2H %.1f ms\n",
                run.ngroups(), ms(t_start, now()), run.t_front, run.t_create, run.t_wait, run.t_d2h);
    return JB_OK;
}

// The request of a single-engine entry for PCM in f64; a byte sink is chosen with one of request_*() below
static jb::SynthRequest batch_request(const jb_engine *e, const char *const *lines, const size_t *line_off,
                                      size_t n_utts, int32_t device, void **out, size_t *n_out)
{
    jb::SynthRequest rq;
    rq.e = e;
    rq.lines = lines;
    rq.line_off = line_off;
    rq.n_utts = n_utts;
    rq.device = device;
    rq.out = out;
    rq.n_out = n_out;
    return rq;
}

// The sink of a request with the PCM type its encoder reads: FLAC and IMA ADPCM 16 bits, the sample formats f64
static jb::SynthRequest &request_flac(jb::SynthRequest &rq, const jb_flac_opts *opts, const jb_flac_meta *meta)
{
    rq.sink = jb::SynthSink::Flac;
    rq.i16 = true;
    rq.flac = opts;
    rq.flac_meta = meta;
    return rq;
}

static jb::SynthRequest &request_formatted(jb::SynthRequest &rq, const jb_format_opts *opts)
{
    rq.sink = jb::SynthSink::Formatted;
    rq.i16 = false;
    rq.fmt = opts;
    return rq;
}

static jb::SynthRequest &request_adpcm(jb::SynthRequest &rq, const jb_adpcm_opts *opts, size_t *n_samples)
{
    rq.sink = jb::SynthSink::Adpcm;
    rq.i16 = true;
    rq.adpcm = opts;
    rq.counts = n_samples;
    return rq;
}

static jb::SynthRequest &request_fbank(jb::SynthRequest &rq, const jb_fbank_opts *opts, size_t *n_frames)
{
    rq.sink = jb::SynthSink::Fbank;
    rq.i16 = false;
    rq.fbank = opts;
    rq.counts = n_frames;
    return rq;
}

static jb::SynthRequest &request_mfcc(jb::SynthRequest &rq, const jb_fbank_opts *fopts, const jb_mfcc_opts *opts,
                                      size_t *n_frames)
{
    request_fbank(rq, fopts, n_frames);
    rq.sink = jb::SynthSink::Mfcc;
    rq.mfcc = opts;
    return rq;
}

static jb::SynthRequest &request_melspec(jb::SynthRequest &rq, const jb_melspec_opts *opts, size_t *n_frames)
{
    rq.sink = jb::SynthSink::Melspec;
    rq.i16 = false;
    rq.melspec = opts;
    rq.counts = n_frames;
    return rq;
}

static jb::SynthRequest &request_pitch(jb::SynthRequest &rq, const jb_pitch_opts *opts, size_t *n_frames)
{
    rq.sink = jb::SynthSink::Pitch;
    rq.i16 = false;
    rq.pitch = opts;
    rq.counts = n_frames;
    return rq;
}

static jb::SynthRequest &request_join(jb::SynthRequest &rq, const jb_join_opts *join, uint64_t *starts)
{
    rq.join = join;
    rq.join_starts = starts;
    return rq;
}

extern "C" {

int jb_synthesize_batch(const jb_engine *e, const char *const *lines, const size_t *line_off,
                        size_t n_utts, int32_t device, double **pcm, size_t *n_samples)
{
    return jb::synthesize_batch_impl(batch_request(e, lines, line_off, n_utts, device, (void **)pcm, n_samples));
}

int jb_synthesize_batch_i16(const jb_engine *e, const char *const *lines, const size_t *line_off,
                            size_t n_utts, int32_t device, int16_t **pcm, size_t *n_samples)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)pcm, n_samples);
    rq.i16 = true;
    return jb::synthesize_batch_impl(rq);
}

void jb_pcm_i16_free(int16_t *p) { free(p); }

} // extern "C"

// The engines of jb_synthesize_batch_each: one voice set (the same Voice objects: jb_engine_new / Engine::clone) and
// the Condition fields one batch cannot vary.  Host-side only, before any device is touched.
static int check_engines(const jb_engine *const *engines, size_t n)
{
    if (!engines) {
        jb::set_error("jb_synthesize_batch_each: engines is NULL");
        return JB_ERR_INVALID;
    }
    for (size_t u = 0; u < n; u++)
        if (!engines[u]) {
            jb::set_error("jb_synthesize_batch_each: engines[" + std::to_string(u) + "] is NULL");
            return JB_ERR_INVALID;
        }
    const jb::Engine &e0 = *CENG(engines[0]);
    for (size_t u = 1; u < n; u++) {
        const jb::Engine &e = *CENG(engines[u]);
        const char *field = nullptr;
        if (e.voices != e0.voices)
            field = "voice set (engines must be made from one another with jb_engine_new)";
        else if (e.cond.sampling_frequency != e0.cond.sampling_frequency)
            field = "sampling_frequency";
        else if (e.cond.fperiod != e0.cond.fperiod)
            field = "fperiod";
        else if (e.cond.stage != e0.cond.stage)
            field = "stage";
        else if (e.cond.use_log_gain != e0.cond.use_log_gain)
            field = "use_log_gain";
        else if (e.cond.batch_invariant != e0.cond.batch_invariant)
            field = "batch_invariant";
        else if (e.cond.fast_invariant != e0.cond.fast_invariant)
            field = "fast_invariant";
        else if (e.cond.tree_search != e0.cond.tree_search)
            field = "tree_search";
        else if (e.cond.loudness_scope != e0.cond.loudness_scope)
            field = "loudness_scope";
        else if (e0.cond.loudness_scope == JB_LOUDNESS_PER_REQUEST) {
            // one gain for the request: what the members of a loudness group must share
            const double a = e.cond.loudness_target, b = e0.cond.loudness_target;
            if (!(a == b || (std::isnan(a) && std::isnan(b))))
                field = "loudness_target (per-request loudness scope)";
            else if (e.cond.peak_ceiling != e0.cond.peak_ceiling)
                field = "peak_ceiling (per-request loudness scope)";
            else if (e.cond.peak_mode != e0.cond.peak_mode)
                field = "peak_mode (per-request loudness scope)";
            else if (e.cond.output_rate != e0.cond.output_rate)
                field = "output_sampling_frequency (per-request loudness scope)";
        }
        if (field) {
            jb::set_error("jb_synthesize_batch_each: engines[" + std::to_string(u) + "] differs from engines[0] in " +
                          field);
            return JB_ERR_INVALID;
        }
    }
    return JB_OK;
}

// rq (its engine fields not yet set) with utterance u under engines[u]
static int synthesize_each(const jb_engine *const *engines, jb::SynthRequest rq)
{
    if (!rq.out || !rq.n_out || (rq.n_utts && !rq.line_off))
        return JB_ERR_INVALID;
    if (rq.n_utts == 0)
        return JB_OK;
    const int rc = check_engines(engines, rq.n_utts);
    if (rc)
        return rc;
    rq.e = engines[0];
    rq.each = engines;
    return jb::synthesize_batch_impl(rq);
}

// The options of the request's sink, under the entry's name (the FLAC checks name their struct instead)
static int check_sink_opts(const jb::SynthRequest &rq, const char *who)
{
    int rc = JB_OK;
    switch (rq.sink) {
    case jb::SynthSink::Pcm:
        return JB_OK;
    case jb::SynthSink::Flac:
        rc = jb::flac_check_opts(rq.flac, nullptr);
        return rc ? rc : jb::flac_check_meta(rq.flac_meta, nullptr);
    case jb::SynthSink::Formatted:
        if (!rq.fmt) {
            jb::set_error(std::string(who) + ": opts is NULL");
            return JB_ERR_INVALID;
        }
        return jb::format_check_opts(rq.fmt->format, rq.fmt->dither, who);
    case jb::SynthSink::Adpcm:
        return jb::adpcm_check_opts((const jb::AdpcmOpts *)rq.adpcm, who);
    case jb::SynthSink::Fbank:
        return jb::fbank_check_opts((const jb::FbankOpts *)rq.fbank, who);
    case jb::SynthSink::Mfcc:
        rc = jb::mfcc_check_fbank((const jb::FbankOpts *)rq.fbank, who);
        return rc ? rc : jb::mfcc_check_opts((const jb::MfccOpts *)rq.mfcc, rq.fbank->n_mels, who);
    case jb::SynthSink::Melspec:
        return jb::mel_check_opts((const jb::MelOpts *)rq.melspec, who);
    case jb::SynthSink::Pitch:
        return jb::pitch_check_opts((const jb::PitchOpts *)rq.pitch, who, nullptr);
    }
    return JB_ERR_INVALID;
}

// jb_synthesize_programme*: the join options
static int check_join_entry(const jb_engine *e, const jb_join_opts *j, size_t n_utts, const char *who)
{
    if (!j) {
        jb::set_error(std::string(who) + ": join is NULL");
        return JB_ERR_INVALID;
    }
    for (double ms : {j->lead_ms, j->gap_ms, j->trail_ms, j->fade_ms})
        if (!(ms >= 0.0) || !std::isfinite(ms)) {
            jb::set_error(std::string(who) + ": lead_ms, gap_ms, trail_ms and fade_ms are finite and not negative");
            return JB_ERR_INVALID;
        }
    if (j->reserved[0] || j->reserved[1]) {
        jb::set_error(std::string(who) + ": reserved must be 0");
        return JB_ERR_INVALID;
    }
    if (n_utts == 0) {
        jb::set_error(std::string(who) + ": a programme has at least one utterance");
        return JB_ERR_INVALID;
    }
    // while jb_engine_set_programme_mix is set the call mixes: one place per utterance, and no gap
    const size_t n_mix = e ? CENG(e)->cond.mix_place.size() : 0;
    if (n_mix && n_mix != n_utts) {
        jb::set_error(std::string(who) + ": jb_engine_set_programme_mix places " + std::to_string(n_mix) +
                      " utterances, the call has " + std::to_string(n_utts));
        return JB_ERR_INVALID;
    }
    if (n_mix && j->gap_ms != 0.0) {
        jb::set_error(std::string(who) + ": gap_ms must be 0 while jb_engine_set_programme_mix is set");
        return JB_ERR_INVALID;
    }
    return JB_OK;
}

// What every byte-sink and programme entry does behind its argument marshalling.  rq carries the sink, its options and
// (programme: a jb_synthesize_programme* entry, which demands one) the join; engines: the _each form, utterance u under
// engines[u].  The sink's options, then the join's, are checked under the entry's name before any device is touched
static int synthesize_entry(const char *who, const jb::SynthRequest &rq, const jb_engine *const *engines,
                            bool programme)
{
    int rc = check_sink_opts(rq, who);
    if (rc || (programme && (rc = check_join_entry(rq.e, rq.join, rq.n_utts, who))))
        return rc;
    return engines ? synthesize_each(engines, rq) : jb::synthesize_batch_impl(rq);
}

extern "C" {

int jb_synthesize_batch_each(const jb_engine *const *engines, const char *const *lines, const size_t *line_off,
                             size_t n_utts, int32_t device, double **pcm, size_t *n_samples)
{
    return synthesize_each(engines, batch_request(nullptr, lines, line_off, n_utts, device, (void **)pcm, n_samples));
}

int jb_synthesize_batch_each_i16(const jb_engine *const *engines, const char *const *lines, const size_t *line_off,
                                 size_t n_utts, int32_t device, int16_t **pcm, size_t *n_samples)
{
    jb::SynthRequest rq = batch_request(nullptr, lines, line_off, n_utts, device, (void **)pcm, n_samples);
    rq.i16 = true;
    return synthesize_each(engines, rq);
}

// The byte sinks' entries: per sink batch, batch_each, single and programme (FLAC: with and without its metadata).
// Each marshals its arguments into a request and goes through synthesize_entry; a single form is its batch form of one
// utterance on the current device, and reports under that name

int jb_synthesize_batch_flac_meta(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                                  int32_t device, const jb_flac_opts *opts, const jb_flac_meta *meta, uint8_t **flac,
                                  size_t *n_bytes)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)flac, n_bytes);
    return synthesize_entry("jb_synthesize_batch_flac_meta", request_flac(rq, opts, meta), nullptr, false);
}

int jb_synthesize_batch_flac(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                             int32_t device, const jb_flac_opts *opts, uint8_t **flac, size_t *n_bytes)
{
    return jb_synthesize_batch_flac_meta(e, lines, line_off, n_utts, device, opts, nullptr, flac, n_bytes);
}

int jb_synthesize_batch_each_flac_meta(const jb_engine *const *engines, const char *const *lines,
                                       const size_t *line_off, size_t n_utts, int32_t device, const jb_flac_opts *opts,
                                       const jb_flac_meta *meta, uint8_t **flac, size_t *n_bytes)
{
    jb::SynthRequest rq = batch_request(nullptr, lines, line_off, n_utts, device, (void **)flac, n_bytes);
    return synthesize_entry("jb_synthesize_batch_each_flac_meta", request_flac(rq, opts, meta), engines, false);
}

int jb_synthesize_batch_each_flac(const jb_engine *const *engines, const char *const *lines, const size_t *line_off,
                                  size_t n_utts, int32_t device, const jb_flac_opts *opts, uint8_t **flac,
                                  size_t *n_bytes)
{
    return jb_synthesize_batch_each_flac_meta(engines, lines, line_off, n_utts, device, opts, nullptr, flac, n_bytes);
}

int jb_synthesize_flac_meta(const jb_engine *e, const char *const *lines, size_t n, const jb_flac_opts *opts,
                            const jb_flac_meta *meta, uint8_t **flac, size_t *n_bytes)
{
    if (!flac || !n_bytes)
        return JB_ERR_INVALID;
    size_t off[2] = {0, n};
    return jb_synthesize_batch_flac_meta(e, lines, off, 1, -1, opts, meta, flac, n_bytes);
}

int jb_synthesize_flac(const jb_engine *e, const char *const *lines, size_t n, const jb_flac_opts *opts,
                       uint8_t **flac, size_t *n_bytes)
{
    return jb_synthesize_flac_meta(e, lines, n, opts, nullptr, flac, n_bytes);
}

int jb_synthesize_programme_flac_meta(const jb_engine *e, const char *const *lines, const size_t *line_off,
                                      size_t n_utts, int32_t device, const jb_flac_opts *opts, const jb_flac_meta *meta,
                                      const jb_join_opts *join, uint8_t **flac, size_t *n_bytes, uint64_t *starts)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)flac, n_bytes);
    request_join(request_flac(rq, opts, meta), join, starts);
    return synthesize_entry("jb_synthesize_programme_flac_meta", rq, nullptr, true);
}

int jb_synthesize_batch_formatted(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                                  int32_t device, const jb_format_opts *opts, uint8_t **bytes, size_t *n_bytes)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_formatted", request_formatted(rq, opts), nullptr, false);
}

int jb_synthesize_batch_each_formatted(const jb_engine *const *engines, const char *const *lines,
                                       const size_t *line_off, size_t n_utts, int32_t device,
                                       const jb_format_opts *opts, uint8_t **bytes, size_t *n_bytes)
{
    jb::SynthRequest rq = batch_request(nullptr, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_each_formatted", request_formatted(rq, opts), engines, false);
}

int jb_synthesize_formatted(const jb_engine *e, const char *const *lines, size_t n, const jb_format_opts *opts,
                            uint8_t **bytes, size_t *n_bytes)
{
    if (!bytes || !n_bytes)
        return JB_ERR_INVALID;
    size_t off[2] = {0, n};
    return jb_synthesize_batch_formatted(e, lines, off, 1, -1, opts, bytes, n_bytes);
}

int jb_synthesize_programme_formatted(const jb_engine *e, const char *const *lines, const size_t *line_off,
                                      size_t n_utts, int32_t device, const jb_format_opts *opts,
                                      const jb_join_opts *join, uint8_t **bytes, size_t *n_bytes, uint64_t *starts)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    request_join(request_formatted(rq, opts), join, starts);
    return synthesize_entry("jb_synthesize_programme_formatted", rq, nullptr, true);
}

int jb_synthesize_batch_adpcm(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                              int32_t device, const jb_adpcm_opts *opts, uint8_t **bytes, size_t *n_bytes,
                              size_t *n_samples)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_adpcm", request_adpcm(rq, opts, n_samples), nullptr, false);
}

int jb_synthesize_batch_each_adpcm(const jb_engine *const *engines, const char *const *lines, const size_t *line_off,
                                   size_t n_utts, int32_t device, const jb_adpcm_opts *opts, uint8_t **bytes,
                                   size_t *n_bytes, size_t *n_samples)
{
    jb::SynthRequest rq = batch_request(nullptr, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_each_adpcm", request_adpcm(rq, opts, n_samples), engines, false);
}

int jb_synthesize_adpcm(const jb_engine *e, const char *const *lines, size_t n, const jb_adpcm_opts *opts,
                        uint8_t **bytes, size_t *n_bytes, size_t *n_samples)
{
    if (!bytes || !n_bytes)
        return JB_ERR_INVALID;
    size_t off[2] = {0, n};
    return jb_synthesize_batch_adpcm(e, lines, off, 1, -1, opts, bytes, n_bytes, n_samples);
}

int jb_synthesize_programme_adpcm(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                                  int32_t device, const jb_adpcm_opts *opts, const jb_join_opts *join, uint8_t **bytes,
                                  size_t *n_bytes, size_t *n_samples, uint64_t *starts)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    request_join(request_adpcm(rq, opts, n_samples), join, starts);
    return synthesize_entry("jb_synthesize_programme_adpcm", rq, nullptr, true);
}

int jb_synthesize_batch_fbank(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                              int32_t device, const jb_fbank_opts *opts, uint8_t **bytes, size_t *n_bytes,
                              size_t *n_frames)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_fbank", request_fbank(rq, opts, n_frames), nullptr, false);
}

int jb_synthesize_batch_each_fbank(const jb_engine *const *engines, const char *const *lines, const size_t *line_off,
                                   size_t n_utts, int32_t device, const jb_fbank_opts *opts, uint8_t **bytes,
                                   size_t *n_bytes, size_t *n_frames)
{
    jb::SynthRequest rq = batch_request(nullptr, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_each_fbank", request_fbank(rq, opts, n_frames), engines, false);
}

int jb_synthesize_fbank(const jb_engine *e, const char *const *lines, size_t n, const jb_fbank_opts *opts,
                        uint8_t **bytes, size_t *n_bytes, size_t *n_frames)
{
    if (!bytes || !n_bytes)
        return JB_ERR_INVALID;
    size_t off[2] = {0, n};
    return jb_synthesize_batch_fbank(e, lines, off, 1, -1, opts, bytes, n_bytes, n_frames);
}

int jb_synthesize_programme_fbank(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                                  int32_t device, const jb_fbank_opts *opts, const jb_join_opts *join, uint8_t **bytes,
                                  size_t *n_bytes, size_t *n_frames, uint64_t *starts)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    request_join(request_fbank(rq, opts, n_frames), join, starts);
    return synthesize_entry("jb_synthesize_programme_fbank", rq, nullptr, true);
}

int jb_synthesize_batch_mfcc(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                             int32_t device, const jb_fbank_opts *fopts, const jb_mfcc_opts *opts, uint8_t **bytes,
                             size_t *n_bytes, size_t *n_frames)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_mfcc", request_mfcc(rq, fopts, opts, n_frames), nullptr, false);
}

int jb_synthesize_batch_each_mfcc(const jb_engine *const *engines, const char *const *lines, const size_t *line_off,
                                  size_t n_utts, int32_t device, const jb_fbank_opts *fopts, const jb_mfcc_opts *opts,
                                  uint8_t **bytes, size_t *n_bytes, size_t *n_frames)
{
    jb::SynthRequest rq = batch_request(nullptr, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_each_mfcc", request_mfcc(rq, fopts, opts, n_frames), engines, false);
}

int jb_synthesize_mfcc(const jb_engine *e, const char *const *lines, size_t n, const jb_fbank_opts *fopts,
                       const jb_mfcc_opts *opts, uint8_t **bytes, size_t *n_bytes, size_t *n_frames)
{
    if (!bytes || !n_bytes)
        return JB_ERR_INVALID;
    size_t off[2] = {0, n};
    return jb_synthesize_batch_mfcc(e, lines, off, 1, -1, fopts, opts, bytes, n_bytes, n_frames);
}

int jb_synthesize_programme_mfcc(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                                 int32_t device, const jb_fbank_opts *fopts, const jb_mfcc_opts *opts,
                                 const jb_join_opts *join, uint8_t **bytes, size_t *n_bytes, size_t *n_frames,
                                 uint64_t *starts)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    request_join(request_mfcc(rq, fopts, opts, n_frames), join, starts);
    return synthesize_entry("jb_synthesize_programme_mfcc", rq, nullptr, true);
}

int jb_synthesize_batch_melspec(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                                int32_t device, const jb_melspec_opts *opts, uint8_t **bytes, size_t *n_bytes,
                                size_t *n_frames)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_melspec", request_melspec(rq, opts, n_frames), nullptr, false);
}

int jb_synthesize_batch_each_melspec(const jb_engine *const *engines, const char *const *lines, const size_t *line_off,
                                     size_t n_utts, int32_t device, const jb_melspec_opts *opts, uint8_t **bytes,
                                     size_t *n_bytes, size_t *n_frames)
{
    jb::SynthRequest rq = batch_request(nullptr, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_each_melspec", request_melspec(rq, opts, n_frames), engines, false);
}

int jb_synthesize_melspec(const jb_engine *e, const char *const *lines, size_t n, const jb_melspec_opts *opts,
                          uint8_t **bytes, size_t *n_bytes, size_t *n_frames)
{
    if (!bytes || !n_bytes)
        return JB_ERR_INVALID;
    size_t off[2] = {0, n};
    return jb_synthesize_batch_melspec(e, lines, off, 1, -1, opts, bytes, n_bytes, n_frames);
}

int jb_synthesize_programme_melspec(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                                    int32_t device, const jb_melspec_opts *opts, const jb_join_opts *join,
                                    uint8_t **bytes, size_t *n_bytes, size_t *n_frames, uint64_t *starts)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    request_join(request_melspec(rq, opts, n_frames), join, starts);
    return synthesize_entry("jb_synthesize_programme_melspec", rq, nullptr, true);
}

int jb_synthesize_batch_pitch(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                              int32_t device, const jb_pitch_opts *opts, uint8_t **bytes, size_t *n_bytes,
                              size_t *n_frames)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_pitch", request_pitch(rq, opts, n_frames), nullptr, false);
}

int jb_synthesize_batch_each_pitch(const jb_engine *const *engines, const char *const *lines, const size_t *line_off,
                                   size_t n_utts, int32_t device, const jb_pitch_opts *opts, uint8_t **bytes,
                                   size_t *n_bytes, size_t *n_frames)
{
    jb::SynthRequest rq = batch_request(nullptr, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    return synthesize_entry("jb_synthesize_batch_each_pitch", request_pitch(rq, opts, n_frames), engines, false);
}

int jb_synthesize_pitch(const jb_engine *e, const char *const *lines, size_t n, const jb_pitch_opts *opts,
                        uint8_t **bytes, size_t *n_bytes, size_t *n_frames)
{
    if (!bytes || !n_bytes)
        return JB_ERR_INVALID;
    size_t off[2] = {0, n};
    return jb_synthesize_batch_pitch(e, lines, off, 1, -1, opts, bytes, n_bytes, n_frames);
}

int jb_synthesize_programme_pitch(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                                  int32_t device, const jb_pitch_opts *opts, const jb_join_opts *join,
                                  uint8_t **bytes, size_t *n_bytes, size_t *n_frames, uint64_t *starts)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)bytes, n_bytes);
    request_join(request_pitch(rq, opts, n_frames), join, starts);
    return synthesize_entry("jb_synthesize_programme_pitch", rq, nullptr, true);
}

int jb_synthesize_programme(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                            int32_t device, const jb_join_opts *join, double **pcm, size_t *n_samples, uint64_t *starts)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)pcm, n_samples);
    return synthesize_entry("jb_synthesize_programme", request_join(rq, join, starts), nullptr, true);
}

// The stems' entries: the engine's mix with a stems request behind it.  Refused before any device is touched without a
// mix (jb_engine_set_programme_mix), without ids, with an unknown flag or an id of n_utts or above
static int stems_entry(const char *who, jb::SynthRequest &rq, const uint32_t *stem_of, uint32_t flags, size_t *n_outputs,
                       jb_stem_report *reports)
{
    auto refuse = [&](const std::string &what) {
        jb::set_error(std::string(who) + ": " + what);
        return JB_ERR_INVALID;
    };
    if (n_outputs)
        *n_outputs = 0;
    if (!rq.e || !n_outputs)
        return JB_ERR_INVALID;
    if (CENG(rq.e)->cond.mix_place.empty())
        return refuse("the engine holds no mix (jb_engine_set_programme_mix comes first)");
    if (!stem_of)
        return refuse("give one stem id per utterance");
    if (flags & ~JB_MIX_STEM_LEVELS)
        return refuse("flags holds an unknown flag");
    for (size_t u = 0; u < rq.n_utts; u++)
        if (stem_of[u] != JB_MIX_NO_STEM && stem_of[u] >= rq.n_utts)
            return refuse("stem_of of utterance " + std::to_string(u) + " (" + std::to_string(stem_of[u]) +
                          "): a stem id is below the number of utterances, or JB_MIX_NO_STEM");
    rq.stem_of = stem_of;
    rq.stem_flags = flags;
    rq.n_outputs = n_outputs;
    rq.stem_reports = reports;
    return synthesize_entry(who, rq, nullptr, true);
}

int jb_synthesize_programme_stems(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                                  int32_t device, const jb_join_opts *join, const uint32_t *stem_of, uint32_t flags,
                                  double **pcm, size_t *n_samples, size_t *n_outputs, jb_stem_report *reports,
                                  uint64_t *starts)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)pcm, n_samples);
    return stems_entry("jb_synthesize_programme_stems", request_join(rq, join, starts), stem_of, flags, n_outputs,
                       reports);
}

int jb_synthesize_programme_stems_flac_meta(const jb_engine *e, const char *const *lines, const size_t *line_off,
                                            size_t n_utts, int32_t device, const jb_flac_opts *opts,
                                            const jb_flac_meta *meta, const jb_join_opts *join, const uint32_t *stem_of,
                                            uint32_t flags, uint8_t **flac, size_t *n_bytes, size_t *n_outputs,
                                            jb_stem_report *reports, uint64_t *starts)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)flac, n_bytes);
    request_join(request_flac(rq, opts, meta), join, starts);
    return stems_entry("jb_synthesize_programme_stems_flac_meta", rq, stem_of, flags, n_outputs, reports);
}

int jb_synthesize_programme_activity(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                                     int32_t device, const jb_join_opts *join, const jb_activity_opts *opts, double **pcm,
                                     size_t *n_samples, uint8_t **labels, uint64_t *T, uint32_t *C, uint64_t *starts)
{
    const char *who = "jb_synthesize_programme_activity";
    if (!labels || !T || !C || !pcm || !n_samples)
        return JB_ERR_INVALID;
    *labels = nullptr;
    *T = 0;
    *C = 0;
    const int rc = jb::act_check_opts((const jb::ActOpts *)opts, who);
    if (rc)
        return rc;
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)pcm, n_samples);
    rq.activity = opts;
    rq.act_out = labels;
    rq.act_T = T;
    rq.act_C = C;
    return synthesize_entry(who, request_join(rq, join, starts), nullptr, true);
}

int jb_synthesize_programme_i16(const jb_engine *e, const char *const *lines, const size_t *line_off, size_t n_utts,
                                int32_t device, const jb_join_opts *join, int16_t **pcm, size_t *n_samples,
                                uint64_t *starts)
{
    jb::SynthRequest rq = batch_request(e, lines, line_off, n_utts, device, (void **)pcm, n_samples);
    rq.i16 = true;
    return synthesize_entry("jb_synthesize_programme_i16", request_join(rq, join, starts), nullptr, true);
}

int jb_synthesize(const jb_engine *e, const char *const *lines, size_t n, double **pcm, size_t *n_samples)
{
    if (!pcm || !n_samples)
        return JB_ERR_INVALID;
    size_t off[2] = {0, n};
    return jb_synthesize_batch(e, lines, off, 1, -1, pcm, n_samples);
}

// ---- generator (src/speech.rs) ----
int jb_generator_new(const jb_engine *e, const char *const *lines, size_t n, jb_generator **out)
{
    if (!e || !out)
        return JB_ERR_INVALID;
    *out = nullptr;
    jb::States st;
    int rc = build_states(*CENG(e), lines, n, st, false, host_threads_default(), nullptr, -1);
    if (rc)
        return rc;
    std::unique_ptr<jb::Generator> g(new jb::Generator());
    jb_batch_opts opts{};
    opts.device = -1;
    opts.flags = CENG(e)->cond.batch_flags();
    if (const char *ev = getenv("JB_GENERATOR_TEST_GANG_TIMEOUT")) // test aid, as JB_BATCH_TEST_GANG_TIMEOUT
        if (atoi(ev) != 0)
            opts.flags |= JB_BATCH_TEST_GANG_TIMEOUT;
    jb::Batch *b = nullptr;
    if ((rc = jb::Batch::create(&CENG(e)->desc, &st.utt, 1, &opts, &b)))
        return rc;
    g->batch.reset(b);
    g->fperiod = b->voice.fperiod;
    g->total = b->T[0];
    if (CENG(e)->cond.output_rate) {
        const uint32_t hz = (uint32_t)CENG(e)->cond.output_rate;
        if ((rc = b->out.set_output_rate(&hz, 1)))
            return rc;
        g->L = b->out.utt(0).L;
        g->M = b->out.utt(0).M;
    }
    if (CENG(e)->cond.filter.n_sections && (rc = b->out.set_filter(&CENG(e)->cond.filter, 1)))
        return rc;
    if (!CENG(e)->cond.fir_taps.empty()) {
        const jb_fir f = CENG(e)->cond.fir();
        if ((rc = b->out.set_fir(&f, 1)))
            return rc;
    }
    if (CENG(e)->cond.room_on) {
        jb_room rm;
        if ((rc = CENG(e)->cond.room(0, &rm)) || (rc = b->out.set_room(&rm, 1)))
            return rc;
    }
    {
        const jb_noise nz = CENG(e)->cond.noise();
        if ((nz.bed || nz.kind != JB_NOISE_BED) && (rc = b->out.set_noise(&nz, 1)))
            return rc;
    }
    if (!std::isnan(CENG(e)->cond.loudness_target)) {
        const double t = CENG(e)->cond.loudness_target, c = CENG(e)->cond.peak_ceiling;
        const uint32_t mode = CENG(e)->cond.peak_mode;
        if ((rc = b->out.set_loudness(&t, &c, 1)) || (rc = b->out.set_peak_mode(&mode, 1)) ||
            (CENG(e)->cond.limiter_on && (rc = b->out.set_limiter(&CENG(e)->cond.limiter, 1))))
            return rc;
    }
    // Engine::generator runs all three MLPGs before returning (src/engine.rs:333-357); here they are
    // enqueued, with the vocoder behind them, and the call returns while the device works
    // (no serially served head with an output rate either: the converted samples of a frame need its successors)
    // (nor with a loudness target: the gain needs every sample; nor with a filter: the chain rewrites the PCM)
    if ((!b->invariant && !b->out.active() && (rc = b->build_generator_work())) || (rc = b->run(false)))
        return rc;
    *out = (jb_generator *)g.release();
    return JB_OK;
}

// SpeechGenerator::new(fperiod, vocoder, spectrum, lf0, lpf) on tracks the caller holds (src/speech.rs:25-50),
// to be stepped with jb_generator_step (generate_step, :65-82): the same three panics as error codes
int jb_generator_new_from_tracks(const jb_voice_desc *voice, const jb_track_utt *utt, const jb_batch_opts *opts,
                                 jb_generator **out)
{
    if (!voice || !utt || !out)
        return JB_ERR_INVALID;
    *out = nullptr;
    std::unique_ptr<jb::Generator> g(new jb::Generator());
    jb_batch_opts o{};
    if (opts)
        o = *opts;
    else
        o.device = -1;
    o.flags &= ~(uint32_t)(JB_BATCH_PCM_I16 | JB_BATCH_MLPG_ONLY); // generate_step hands out f64 samples
    jb::Batch *b = nullptr;
    jb::TrackSrc src{utt};
    int rc = jb::Batch::create(voice, nullptr, 1, &o, &b, nullptr, &src);
    if (rc)
        return rc;
    g->batch.reset(b);
    g->fperiod = b->voice.fperiod;
    g->total = b->T[0];
    if ((!b->invariant && (rc = b->build_generator_work())) || (rc = b->run(false)))
        return rc;
    *out = (jb_generator *)g.release();
    return JB_OK;
}

size_t jb_generator_fperiod(const jb_generator *g) { return g ? ((const jb::Generator *)g)->fperiod : 0; }
size_t jb_generator_synthesized_frames(const jb_generator *g)
{
    return g ? ((const jb::Generator *)g)->next : 0;
}
size_t jb_generator_total_frames(const jb_generator *g) { return g ? ((const jb::Generator *)g)->total : 0; }

// waits for the whole-utterance run (and its certification / redo) once
static int generator_finish(jb::Generator *g)
{
    if (g->ahead_ready)
        return JB_OK;
    int rc = g->batch->sync();
    if (rc)
        return rc;
    g->ahead_ready = true;
    return JB_OK;
}

// Output rate / loudness target: the converted (normalized) utterance, read whole by the first step, handed out by the steps' ceil rule
static long generator_out(jb::Generator *g, double *buf, size_t buf_len, size_t max_frames)
{
    if (buf_len < g->out_step_max() || !buf) {
        set_error("The length of speech buffer must be at least ceil(fperiod * output rate / voice rate).");
        return JB_ERR_BUFFER;
    }
    jb::Batch *b = g->batch.get();
    if (hipSetDevice(b->device) != hipSuccess)
        return JB_ERR_DEVICE;
    int rc = generator_finish(g);
    if (rc)
        return rc;
    if (g->cache.empty() && b->out.samples(0)) {
        g->cache.resize(b->out.samples(0));
        if ((rc = b->read(b->out.pcm64() + b->out.offset(0), g->cache.data(), g->cache.size() * sizeof(double), false)))
            return rc;
    }
    const size_t lo = g->out_start(g->next);
    size_t nf = 0;
    while (nf < max_frames && g->next + nf < g->total && g->out_start(g->next + nf + 1) - lo <= buf_len)
        nf++;
    const size_t hi = std::min(g->out_start(g->next + nf), g->cache.size());
    if (hi > lo)
        memcpy(buf, g->cache.data() + lo, (hi - lo) * sizeof(double));
    g->next += nf;
    return (long)(hi > lo ? hi - lo : 0);
}

long jb_generator_step(jb_generator *hg, double *buf, size_t buf_len)
{
    jb::Generator *g = (jb::Generator *)hg;
    if (!g)
        return JB_ERR_INVALID;
    if (g->total <= g->next)
        return 0;
    if (g->batch->out.active())
        return generator_out(g, buf, buf_len, 1);
    if (buf_len < g->fperiod || !buf) {
        set_error("The length of speech buffer must be larger than fperiod.");
        return JB_ERR_BUFFER;
    }
    jb::Batch *b = g->batch.get();
    if (hipSetDevice(b->device) != hipSuccess)
        return JB_ERR_DEVICE;
    int rc;
    // (no serial head in the fast batch-invariant mode: its frames would not have the bits of jb_synthesize)
    if (!g->ahead_ready &&
        (g->next >= kGenSerialFrames || !b->gen_work_dev || hipEventQuery(b->ev_voc_done) == hipSuccess) &&
        (rc = generator_finish(g)))
        return rc;
    if (!g->ahead_ready) {
        // the utterance is still in flight: this frame from the serial recursion on the side stream
        hipStream_t ss = b->stream_lf0;
        hipError_t he;
        if (!g->serial_armed) {
            // Parameter generation must be complete before a frame is served -- and it is not if the resident GV
            // kernel gave up in formation (possible without a fault when several such launches share a device:
            // generators made back to back): the flag is read here, once, not only in Batch::sync, which would
            // redo the step after the head of the utterance had gone out computed from an unfinished MCP track.
            if ((he = hipEventSynchronize(b->ev_mlpg_done)) != hipSuccess)
                return hip_fail(he, "generator: parameter generation");
            bool timed_out = false;
            if ((rc = b->gang_timeout_seen(&timed_out)))
                return rc;
            if (timed_out) {
                if ((rc = generator_finish(g))) // sync(): the step again with the multi-launch GV, certified
                    return rc;
            } else {
                g->serial_armed = true;
            }
        }
        if (g->serial_armed && !g->ahead_ready) {
            // the serial recursion writes the frame into a buffer of its own (the whole-utterance run is writing
            // the same frames of the PCM slab, and from the throughput kernel not bit for bit the same values)
            jb::VocDev vdg = b->vd;
            vdg.pcm = b->gen_pcm - g->next * g->fperiod; // utterance 0, frame `next` -> gen_pcm[0 .. fperiod)
            if ((he = launch_vocoder(b->bd, vdg, b->gen_work_dev + g->next, 1, ss)) != hipSuccess)
                return hip_fail(he, "k_vocoder");
            if ((he = hipStreamSynchronize(ss)) != hipSuccess)
                return hip_fail(he, "generator step");
            if ((rc = b->read(b->gen_pcm, buf, g->fperiod * sizeof(double), false)))
                return rc;
            g->next++;
            return (long)g->fperiod;
        }
    }
    if (g->next < g->cache_first || g->next >= g->cache_first + g->cache_frames) {
        const size_t nf = std::min(kGenBlockFrames, g->total - g->next);
        g->cache.resize(nf * g->fperiod);
        if ((rc = b->read(b->vd.pcm + g->next * g->fperiod, g->cache.data(), nf * g->fperiod * sizeof(double), false)))
            return rc;
        g->cache_first = g->next;
        g->cache_frames = nf;
    }
    memcpy(buf, g->cache.data() + (g->next - g->cache_first) * g->fperiod, g->fperiod * sizeof(double));
    g->next++;
    return (long)g->fperiod;
}

long jb_generator_step_n(jb_generator *hg, double *buf, size_t buf_len, size_t max_frames)
{
    jb::Generator *g = (jb::Generator *)hg;
    if (!g)
        return JB_ERR_INVALID;
    if (g->total <= g->next || max_frames == 0)
        return 0;
    if (g->batch->out.active())
        return generator_out(g, buf, buf_len, max_frames);
    if (buf_len < g->fperiod || !buf) {
        set_error("The length of speech buffer must be larger than fperiod.");
        return JB_ERR_BUFFER;
    }
    const size_t nf = std::min(std::min(max_frames, g->total - g->next), buf_len / g->fperiod);
    jb::Batch *b = g->batch.get();
    if (hipSetDevice(b->device) != hipSuccess)
        return JB_ERR_DEVICE;
    int rc = generator_finish(g);
    if (rc)
        return rc;
    if ((rc = b->read(b->vd.pcm + g->next * g->fperiod, buf, nf * g->fperiod * sizeof(double), false)))
        return rc;
    g->next += nf;
    return (long)(nf * g->fperiod);
}

void jb_generator_free(jb_generator *g) { delete (jb::Generator *)g; }

} // extern "C"
