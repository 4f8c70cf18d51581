// jb_treesearch.h -- the decision trees of a voice set as flat tables, and a scalar walker over them.
//
// Engine-level synthesis searches, for every label, the duration tree and the nstream x nstate stream trees of every
// voice (Model::get_index, jb_voice.h) and tests the GV switch question.  The tables below hold everything that
// search reads -- pattern text, compiled patterns, questions, tree nodes -- in index arrays without pointers, so that
// the same bytes serve the host walker (ts_walk_label, jb_treesearch.cpp) and the device kernel (jb_treesearch.hip).
// Pure host: nothing here touches a device.
#pragma once
#include <cstdint>
#include <memory>
#include <string_view>
#include <vector>

namespace jb {

struct Voice;

// kind: Question::Kind (Glob, Contains, Prefix, Suffix, Exact, Any); the text is pool[off .. off + len): the whole
// pattern for Glob, the literal core otherwise (Question::compile)
struct TsPattern {
    uint32_t kind, off, len;
};
struct TsQuestion {
    uint32_t first, n;           // patterns [first, first + n): the question is their OR
    uint32_t text_off, text_len; // their text, contiguous in the pool (the kernel fetches it in one load)
};
// question: index into TsTables::questions (every model's questions are concatenated, so an index names a (model,
// question) pair); yes / no as TreeNode: >= 0 the node's index within its tree, < 0 a leaf with pdf index -value
struct TsNode {
    int32_t question, yes, no;
};
struct TsTree {
    int32_t root;     // first node in TsTables::nodes; -1: an empty tree, whose answer is `leaf` (Tree::single_leaf)
    int32_t leaf;
    uint32_t n_nodes;
    int32_t state;    // Tree::state
    uint32_t npdf;    // Model::npdf of the tree
    uint32_t row_off; // rows of the model's earlier trees (Engine::CatTable::tree_off)
};
struct TsModel {
    uint32_t tree0, n_trees; // trees [tree0, tree0 + n_trees) of TsTables::trees, in the model's order
};

constexpr uint32_t kTsMaxLabel = 1023; // bytes of a label the device search takes

struct TsTables {
    // model (v, k) = v * nkind + k: kind 0 the duration model, kind 1 + si stream si
    uint32_t nv = 0, nkind = 0, nstate = 0;
    uint32_t gv_question = 0; // voice 0's GV_OFF_CONTEXT question (the last one)
    std::vector<uint8_t> pool;
    std::vector<TsPattern> patterns;
    std::vector<TsQuestion> questions;
    std::vector<TsNode> nodes;
    std::vector<TsTree> trees;
    std::vector<TsModel> models;
    // [model][nstate]: position (within the model) of the first tree whose state is 2 + s, -1 when there is none
    // (get_index then searches tree 0 and reports the position -1).  The duration model has one state index, 2:
    // its entries s > 0 are never searched
    std::vector<int32_t> state_tree;
    size_t entries() const { return (size_t)nv * nkind * nstate; } // results per label
};

// The tables as the device sees them (pointers into one device block; jb_engine.cpp owns it)
struct TsDev {
    const uint8_t *pool;
    const TsPattern *patterns;
    const TsQuestion *questions;
    const TsNode *nodes;
    const TsTree *trees;
    const TsModel *models;
    const int32_t *state_tree;
    uint32_t nv, nkind, nstate, gv_question;
    uint32_t memo_words; // 32-bit words of a label's answer memo (two bits per question); 0: no memo
};

void ts_flatten(const std::vector<std::shared_ptr<Voice>> &voices, size_t nstream, TsTables *out);
bool ts_question(const TsTables &t, uint32_t question, std::string_view label);
// One label: tree_pos / pdf_index [nv][nkind][nstate] -- entry (v, 0, 0) the duration tree, (v, 0, s > 0) = -1 / 0,
// (v, 1 + si, s) stream si at state index 2 + s; each the pair Model::get_index returns -- and gv_on =
// !gv_off.test(label).  memo: scratch the walker sizes itself, kept by the caller from label to label.
// A walk that does not end within the tree's node count (a leaf numbered 0 reads as node 0: Tree::search never
// returns from such a cycle) gives pdf index 0.
void ts_walk_label(const TsTables &t, std::string_view label, int32_t *tree_pos, int32_t *pdf_index, uint8_t *gv_on,
                   std::vector<int8_t> &memo);

} // namespace jb
