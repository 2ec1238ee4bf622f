// graph_cache.h -- a model's captured steps: one capture helper and a capped
// cache of graph executables keyed by step shape.
#pragma once
#include <map>

#include "../ffmi_internal.h"

namespace ffmi {

// Captures what enqueue() puts on `stream` (thread-local mode: other threads'
// models go on making HIP calls) and instantiates it into *out.  The graph is
// destroyed on every path.  enqueue's own failure is returned first, a HIP
// error (left as the last error) otherwise.
template <typename Enqueue>
ffmi_status capture_graph(hipStream_t stream, Enqueue &&enqueue, hipGraphExec_t *out) {
  hipGraph_t g = nullptr;
  FFMI_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
  const ffmi_status st = enqueue();
  const hipError_t ce = hipStreamEndCapture(stream, &g);
  if (st != FFMI_OK || ce != hipSuccess) {
    if (g) (void)hipGraphDestroy(g);
    if (st != FFMI_OK) return st;
    FFMI_HIP(ce);
  }
  const hipError_t ie = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  FFMI_HIP(ie);
  return FFMI_OK;
}

// Executables by key, at most `cap` of them: the owner clears a full cache
// before it captures another (step shapes recur; nothing is worth ranking),
// and clears it before its stream goes away.
template <typename Key>
struct GraphCache {
  explicit GraphCache(size_t cap) : cap(cap) {}
  hipGraphExec_t find(const Key &key) const {
    const auto it = map.find(key);
    return it == map.end() ? nullptr : it->second;
  }
  bool full() const { return map.size() >= cap; }
  void insert(const Key &key, hipGraphExec_t ex) { map.emplace(key, ex); }
  void clear() {
    for (auto &kv : map) (void)hipGraphExecDestroy(kv.second);
    map.clear();
  }

 private:
  size_t cap;
  std::map<Key, hipGraphExec_t> map;
};

}  // namespace ffmi
