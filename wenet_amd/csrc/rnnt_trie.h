// Prefix trie of one utterance's hypotheses, for the teacher-forced transducer score
// (transducer_score.hip).  Plain C++: no HIP call, no device -- it compiles and runs on a CPU.
//
// A column u of a hypothesis' RNN-T lattice depends only on the prefix y[:u]: it reads the joint
// row of that prefix at the columns `blank` and y[u].  Hypotheses of one n-best share most of
// their prefixes, so the joint is evaluated once per (frame, trie node), not once per
// (frame, hypothesis, u).
//   node 0            the empty prefix (predictor input [blank]); parent -1, token blank, depth 0
//   every other node  parent, token, depth; nodes are in LEVEL order (all of depth d before any
//                     of depth d + 1), within a level in order of first appearance when the
//                     hypotheses are scanned in their given order: parents precede children
//   slot[i]           place of node i's token in its parent's column list (>= 1; 0 for node 0)
//   path              per hypothesis its len + 1 node ids (path_off: n + 1 offsets)
//   cols              per node (col_off: nodes + 1 offsets) the joint columns it is read at: the
//                     blank first, then its children's tokens in node order
#pragma once
#include <vector>

namespace wn {

struct RnntTrie {
  std::vector<int> parent, token, depth, slot;
  std::vector<int> path, path_off;
  std::vector<int> col_off, cols;
  int nodes() const { return (int)parent.size(); }
};

// hypothesis k of n: lens[k] tokens at tokens + k * pitch
inline void rnnt_trie_build(const int* tokens, const int* lens, int n, int pitch, int blank,
                            RnntTrie& t) {
  t.parent.assign(1, -1);
  t.token.assign(1, blank);
  t.depth.assign(1, 0);
  t.slot.assign(1, 0);
  std::vector<std::vector<int>> kids(1), paths(n, std::vector<int>(1, 0));
  std::vector<int> cur(n, 0);
  int longest = 0;
  for (int k = 0; k < n; ++k) longest = lens[k] > longest ? lens[k] : longest;
  for (int d = 1; d <= longest; ++d) {
    for (int k = 0; k < n; ++k) {
      if (lens[k] < d) continue;
      const int tok = tokens[(size_t)k * pitch + d - 1], p = cur[k];
      int c = -1;
      for (size_t i = 0; i < kids[p].size() && c < 0; ++i)
        if (t.token[kids[p][i]] == tok) c = kids[p][i];
      if (c < 0) {
        c = t.nodes();
        t.parent.push_back(p);
        t.token.push_back(tok);
        t.depth.push_back(d);
        t.slot.push_back((int)kids[p].size() + 1);
        kids[p].push_back(c);
        kids.emplace_back();
      }
      cur[k] = c;
      paths[k].push_back(c);
    }
  }
  t.path.clear();
  t.path_off.assign(1, 0);
  for (int k = 0; k < n; ++k) {
    t.path.insert(t.path.end(), paths[k].begin(), paths[k].end());
    t.path_off.push_back((int)t.path.size());
  }
  t.cols.clear();
  t.col_off.assign(1, 0);
  for (int i = 0; i < t.nodes(); ++i) {
    t.cols.push_back(blank);
    for (int c : kids[i]) t.cols.push_back(t.token[c]);
    t.col_off.push_back((int)t.cols.size());
  }
}

// A stateless predictor's window of every node, ctx + node * C, oldest first: the last C entries
// of [-1, ..., -1, blank, the path to the node] (node 0's token is the blank).
inline void rnnt_trie_context(const RnntTrie& t, int C, int* ctx) {
  for (int i = 0; i < t.nodes(); ++i) {
    int c = C - 1;
    for (int j = i; c >= 0 && j >= 0; j = t.parent[j]) ctx[(size_t)i * C + c--] = t.token[j];
    for (; c >= 0; --c) ctx[(size_t)i * C + c] = -1;
  }
}

}  // namespace wn
