// jb_treesearch.cpp -- flattens a voice set's decision trees (jb_treesearch.h) and walks the flat tables on the
// host.  The walker reads nothing but the tables, as the kernel of jb_treesearch.hip does: a test that compares it
// with Model::get_index checks the flattening and the matcher on a machine without a GPU.
#include "jb_treesearch.h"
#include "jb_voice.h"

#include <cstring>

namespace jb {

namespace {

uint32_t add_question(const Question &q, TsTables *t)
{
    // (a question that was never compiled goes through the general matcher, as Question::test does)
    const bool compiled = q.compiled.size() == q.patterns.size();
    TsQuestion rec{(uint32_t)t->patterns.size(), (uint32_t)q.patterns.size(), (uint32_t)t->pool.size(), 0};
    for (size_t i = 0; i < q.patterns.size(); i++) {
        const std::string &text = compiled ? q.compiled[i].second : q.patterns[i];
        const uint32_t kind = compiled ? (uint32_t)q.compiled[i].first : (uint32_t)Question::Glob;
        t->patterns.push_back(TsPattern{kind, (uint32_t)t->pool.size(), (uint32_t)text.size()});
        t->pool.insert(t->pool.end(), text.begin(), text.end());
    }
    rec.text_len = (uint32_t)t->pool.size() - rec.text_off;
    t->questions.push_back(rec);
    return (uint32_t)t->questions.size() - 1;
}

void add_model(const Model &m, int n_states_searched, TsTables *t)
{
    const uint32_t q0 = (uint32_t)t->questions.size();
    for (const Question &q : m.questions)
        add_question(q, t);
    TsModel rec{(uint32_t)t->trees.size(), (uint32_t)m.trees.size()};
    uint32_t row_off = 0;
    for (size_t k = 0; k < m.trees.size(); k++) {
        const Tree &tr = m.trees[k];
        TsTree o{};
        o.root = tr.nodes.empty() ? -1 : (int32_t)t->nodes.size();
        o.leaf = tr.single_leaf;
        o.n_nodes = (uint32_t)tr.nodes.size();
        o.state = tr.state;
        o.npdf = k < m.npdf.size() ? (uint32_t)m.npdf[k] : 0u;
        o.row_off = row_off;
        row_off += o.npdf;
        for (const TreeNode &n : tr.nodes)
            t->nodes.push_back(TsNode{(int32_t)q0 + n.question, n.yes, n.no});
        t->trees.push_back(o);
    }
    t->models.push_back(rec);
    for (uint32_t s = 0; s < t->nstate; s++) {
        int32_t pos = -1;
        for (size_t k = 0; (int)s < n_states_searched && k < m.trees.size(); k++)
            if (m.trees[k].state == (int)(2 + s)) {
                pos = (int32_t)k;
                break;
            }
        t->state_tree.push_back(pos);
    }
}

// glob_match (jb_voice.cpp) over the pool's bytes: byte-wise, '?' is one byte
bool glob_bytes(const uint8_t *pat, uint32_t np, const char *s, size_t n)
{
    size_t p = 0, i = 0, star = (size_t)-1, mark = 0;
    while (i < n) {
        if (p < np && (pat[p] == '?' || (pat[p] != '*' && pat[p] == (uint8_t)s[i]))) {
            p++;
            i++;
        } else if (p < np && pat[p] == '*') {
            star = p++;
            mark = i;
        } else if (star != (size_t)-1) {
            p = star + 1;
            i = ++mark;
        } else {
            return false;
        }
    }
    while (p < np && pat[p] == '*')
        p++;
    return p == np;
}

} // namespace

void ts_flatten(const std::vector<std::shared_ptr<Voice>> &voices, size_t nstream, TsTables *out)
{
    TsTables t;
    t.nv = (uint32_t)voices.size();
    t.nkind = (uint32_t)(1 + nstream);
    t.nstate = voices.empty() ? 0u : (uint32_t)voices[0]->meta.num_states;
    for (const auto &v : voices) {
        add_model(v->duration, 1, &t);
        for (size_t si = 0; si < nstream; si++)
            add_model(v->streams[si].stream, (int)t.nstate, &t);
    }
    t.gv_question = voices.empty() ? 0u : add_question(voices[0]->gv_off, &t);
    *out = std::move(t);
}

bool ts_question(const TsTables &t, uint32_t question, std::string_view label)
{
    const TsQuestion &q = t.questions[question];
    const size_t L = label.size();
    for (uint32_t i = q.first; i < q.first + q.n; i++) {
        const TsPattern &p = t.patterns[i];
        const uint8_t *text = t.pool.data() + p.off;
        bool hit = false;
        switch (p.kind) {
        case Question::Any: hit = true; break;
        case Question::Contains:
            for (size_t s = 0; !hit && s + p.len <= L; s++)
                hit = memcmp(label.data() + s, text, p.len) == 0;
            break;
        case Question::Prefix: hit = L >= p.len && memcmp(label.data(), text, p.len) == 0; break;
        case Question::Suffix: hit = L >= p.len && memcmp(label.data() + (L - p.len), text, p.len) == 0; break;
        case Question::Exact: hit = L == p.len && memcmp(label.data(), text, p.len) == 0; break;
        default: hit = glob_bytes(text, p.len, label.data(), L); break;
        }
        if (hit)
            return true;
    }
    return false;
}

void ts_walk_label(const TsTables &t, std::string_view label, int32_t *tree_pos, int32_t *pdf_index, uint8_t *gv_on,
                   std::vector<int8_t> &memo)
{
    memo.assign(t.questions.size(), (int8_t)-1);
    auto ask = [&](uint32_t q) {
        int8_t &c = memo[q];
        if (c < 0)
            c = ts_question(t, q, label) ? 1 : 0;
        return c != 0;
    };
    for (uint32_t m = 0; m < t.nv * t.nkind; m++) {
        const TsModel &mod = t.models[m];
        const bool duration = m % t.nkind == 0;
        for (uint32_t s = 0; s < t.nstate; s++) {
            const size_t e = (size_t)m * t.nstate + s;
            tree_pos[e] = -1;
            pdf_index[e] = 0;
            if ((duration && s > 0) || mod.n_trees == 0)
                continue;
            const int32_t pos = t.state_tree[e];
            tree_pos[e] = pos;
            const TsTree &tr = t.trees[mod.tree0 + (uint32_t)(pos < 0 ? 0 : pos)];
            if (tr.root < 0) {
                pdf_index[e] = tr.leaf;
                continue;
            }
            int32_t i = 0;
            for (uint32_t step = 0; step < tr.n_nodes; step++) {
                const TsNode &n = t.nodes[(size_t)tr.root + (size_t)i];
                const int32_t next = ask((uint32_t)n.question) ? n.yes : n.no;
                if (next < 0) {
                    pdf_index[e] = -next;
                    break;
                }
                i = next;
            }
        }
    }
    if (gv_on)
        *gv_on = !ask(t.gv_question);
}

} // namespace jb
