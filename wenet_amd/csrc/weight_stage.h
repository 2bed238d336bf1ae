// Weight ingestion shared by the wn_model_create* entry points (cabi_model.hip,
// cabi_paraformer.hip): the caller's named tensors (`Src`), the host image of the weight slab
// they are copied / re-laid-out into (`HostStage`), and the fbank tables every handle carries.
#pragma once
#include "model_state.h"
#include "fbank_tables.h"

namespace wn {

struct HostStage {
  std::vector<float> data;
  std::map<std::string, std::pair<size_t, size_t>> at;  // name -> (offset, n)
  void add(const std::string& name, const float* p, size_t n) {
    size_t o = (data.size() + 63) / 64 * 64;
    data.resize(o + n);
    memcpy(data.data() + o, p, n * sizeof(float));
    at[name] = {o, n};
  }
  float* alloc(const std::string& name, size_t n) {
    size_t o = (data.size() + 63) / 64 * 64;
    data.resize(o + n, 0.f);
    at[name] = {o, n};
    return data.data() + o;  // valid until the next add/alloc
  }
};

struct Src {
  std::map<std::string, std::pair<const float*, int64_t>> t;
  const float* get(const std::string& n, int64_t numel) const {
    auto it = t.find(n);
    if (it == t.end()) { set_error("missing weight: " + n); return nullptr; }
    if (numel >= 0 && it->second.second != numel) {
      set_error("weight " + n + " has " + std::to_string(it->second.second) +
                " elements, expected " + std::to_string(numel));
      return nullptr;
    }
    return it->second.first;
  }
  bool has(const std::string& n) const { return t.count(n) != 0; }
};

#define WN_GET(var, name, numel)                 \
  const float* var = src.get((name), (numel));   \
  if (!var) return -3;

inline int stage_linear(const Src& src, HostStage& hs, const std::string& pfx, int out, int in,
                        bool bias = true) {
  WN_GET(w, pfx + ".weight", (int64_t)out * in);
  hs.add(pfx + ".weight", w, (size_t)out * in);
  if (bias) {
    WN_GET(b, pfx + ".bias", out);
    hs.add(pfx + ".bias", b, out);
  }
  return 0;
}
inline int stage_norm(const Src& src, HostStage& hs, const std::string& pfx, int n) {
  WN_GET(w, pfx + ".weight", n);
  WN_GET(b, pfx + ".bias", n);
  hs.add(pfx + ".weight", w, n);
  hs.add(pfx + ".bias", b, n);
  return 0;
}

// the fbank tables into the host image (window, twiddle, mel weights: in this order) ...
inline void stage_fbank_tables(const FbankTables& t, HostStage& hs, ModelData& W) {
  hs.add("fbank.window", t.window.data(), t.window.size());
  hs.add("fbank.twiddle", t.twiddle.data(), t.twiddle.size());
  hs.add("fbank.mel_w", t.mel_w.data(), t.mel_w.size());
  if (!t.ok) W.fbank_ok = false;   // e.g. 128 bins
}
// ... and, once the slab is uploaded and W.w filled, the pointers and the integer table
inline int bind_fbank_tables(const FbankTables& t, ModelData& W) {
  W.fb_window = W.w.at("fbank.window"); W.fb_twiddle = W.w.at("fbank.twiddle");
  W.fb_mel_w = W.w.at("fbank.mel_w");
  std::vector<int> tab;
  tab.insert(tab.end(), t.mel_start.begin(), t.mel_start.end());
  tab.insert(tab.end(), t.mel_len.begin(), t.mel_len.end());
  tab.insert(tab.end(), t.mel_off.begin(), t.mel_off.end());
  WN_TRY(W.fb_tab_i.ensure(tab.size() * sizeof(int)));
  WN_HIP(hipMemcpy(W.fb_tab_i.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace wn
