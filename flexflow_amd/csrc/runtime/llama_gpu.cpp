// llama_gpu.cpp -- LLaMA on MI355X through the C-ABI kernels.
//
// Graph per layer (inference/models/llama.cc:55-252):
//   [rms_norm | residual_rms_norm] -> qkv_proj -> {Inc,Spec,Tree}IncMHA
//   -> o_proj -> AllReduce -> residual_rms_norm -> gate|up (+SiLU-mul fused)
//   -> down_proj -> AllReduce
// tail: residual_rms_norm "norm" -> lm_head -> softmax+argmax (LLM) or
// softmax+arg_top_k (SSM, llama.cc:277-295).
// Tensor parallelism (model.cc:3392-3613, linear.cc:1691-1730): qkv/gate/up
// column-parallel (heads / FFN columns of shard `tp_rank`), o/down
// row-parallel followed by a sum all-reduce -- the direct xGMI transport
// (collective.hip) or RCCL, both in two column halves overlapped on a second
// stream and captured in the step's HIP graph; norms replicated; lm_head
// vocab-sharded with the sharded softmax / top-k tail (model.cc:3392-3419).
#include <dirent.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "graph_cache.h"
#include "model.h"
#include "request_manager.h"  // (now_us)

// return a failed status to the caller
#define TRY(x) \
  do { const ffmi_status st_ = (x); if (st_ != FFMI_OK) return st_; } while (0)

namespace ffmi {

namespace {

struct Layer {
  uint16_t *in_norm = nullptr, *post_norm = nullptr;
  uint16_t *wqkv = nullptr, *wo = nullptr, *wgu = nullptr, *wd = nullptr;
  ffmi_attn *attn = nullptr;
};

// One step as enqueue sees it: the staging batch and result slot it runs on
// (slot 0 unless a chained beam step), its rows, results per row, and the
// bytes of its staged blob.  Built on the stack by whoever launches the step.
struct Step {
  ffmi_batch_dev *batch;
  int slot, T, k;
  size_t blob_bytes;
};

// A per-row side array of a step (4-byte elements): filled from the batch the
// scheduler built, appended to the step's staged blob at `off` (stage_extra)
template <typename E>
struct StepExtra {
  static_assert(sizeof(E) == 4, "4-byte elements");
  std::vector<E> v;
  size_t off = 0;
};

struct LlamaGPU : public ffmi_model {
  ffmi_llama_config c{};
  ffmi_model_opts o{};
  int token_capacity() const override { return o.max_tokens; }
  bool uses_collectives() const override { return o.tp_size > 1; }
  std::string weights_folder;  // reference-format checkpoint ("" = synthetic)
  int Hl = 0, Fl = 0, d = 0, heads_l = 0, slots = 0;
  int Tm = 0;  // max_tokens in whole 16-row groups (packed tiles cover them)
  // FFMI_MODEL_NATIVE_GQA with num_kv_heads < num_heads: this rank's K/V heads,
  // their width and the qkv row [Hl | Hkv | Hkv]; otherwise K/V are (or are
  // replicated to) heads_l heads: kvh_l = heads_l, Hkv = Hl, Nqkv = 3 Hl
  bool native_gqa = false;
  int kvh_l = 0, Hkv = 0, Nqkv = 0;
  // GEMM inputs (normed hidden, attention output, SiLU output) are kept in
  // packed activation tiles: every GEMM then reads its activation fragments
  // as contiguous 1 KiB blocks, like the weights (see act_packed_off)
  bool packed = false;
  // FFMI_W_STREAM on every GEMM when this rank's weights outgrow the 256 MiB
  // Infinity Cache (LLaMA-7B: 13.5 GB streamed once per step; the 68M SSM's
  // 87 MB stay cached from step to step and keep the default policy)
  int wstream = 0;
  hipStream_t stream = nullptr;
  std::vector<Layer> layers;
  uint16_t *embed = nullptr, *final_norm = nullptr, *lm = nullptr;
  // activations
  uint16_t *res = nullptr, *h = nullptr, *qkv = nullptr, *att = nullptr, *proj = nullptr,
           *mlp = nullptr, *logits = nullptr;
  int32_t *ids_d = nullptr;
  // softmax top-k workspace (the split-row form for small steps; zeroed once)
  void *topk_ws = nullptr;
  size_t topk_ws_bytes = 0;
  // top-p sampling (ffmi_model_set_sampling; llama.cc:286-289) instead of the
  // greedy tail.  The host draws one uniform per row, u = (ffmi_sampling_
  // counter(seed, request guid, position of the token produced) + 1) * 2^-24,
  // and appends them to the step's blob behind its records (step_u.off), so
  // they ride the step's one upload and a graph replay reads fresh values
  bool sampling = false;
  float temperature = 0.8f, topp = 0.6f;
  uint64_t sampling_seed = 0;
  // [Tm][V] keys, or, under a vocab-sharded lm_head, the scratch of
  // ffmi_vocab_shard_sample_topp ([Tm][Vl] keys + exchange records);
  // allocated when sampling is first turned on
  uint16_t *sample_ws = nullptr;
  size_t sample_ws_bytes = 0;
  StepExtra<float> step_u;
  ffmi_status set_sampling(bool on, float temp, float p, uint64_t seed) override {
    const char *why = mode != FFMI_MODEL_INC
                          ? "sampling: a BEAM / TREE model decodes greedily (a sampled pick "
                            "cannot verify a greedy token tree)"
                          : Vl != c.vocab_size && !o.comm ? "sampling: vocab-sharded lm_head"
                                                          : nullptr;
    if (why) return refuse(why);
    if (on && !sample_ws) {
      sample_ws_bytes = Vl != c.vocab_size ? ffmi_vocab_shard_sample_scratch_bytes(
                                                 ffmi::comm_size(o.comm), Tm, Vl)
                                           : ffmi::sample_topp_workspace_bytes(Tm, Vl);
      const ffmi_status st = alloc(&sample_ws, (sample_ws_bytes + 1) / 2);
      if (st != FFMI_OK) return st;
    }
    // (the captured graphs hold the tail's kernel and its scalar arguments)
    FFMI_HIP(hipStreamSynchronize(stream));
    clear_graphs();
    sampling = on;
    temperature = temp, topp = p, sampling_seed = seed;
    return FFMI_OK;
  }
  // the step's draws, from the batch the scheduler built
  void draw_step_u(const BatchConfig &bc) {
    step_u.v.resize(bc.num_tokens);
    for (int t = 0; t < bc.num_tokens; ++t) {
      const auto &ti = bc.tokensInfo[t];
      const uint32_t ctr = ffmi_sampling_counter(
          sampling_seed, bc.requestsInfo[ti.request_index].request_guid, ti.abs_depth_in_request + 1);
      step_u.v[t] = (float)(ctr + 1u) * (1.0f / 16777216.0f);
    }
  }
  // per-token log-probabilities (ffmi_model_set_logprobs): ffmi_token_logprobs
  // behind the pick, in the same stream and captured graph.  The rows' targets
  // (BatchConfig::PerTokenInfo::score_id) ride the blob behind the records and
  // the draws, as step_u does, so a replayed graph reads fresh ones; the
  // results go to pinned lp_h.  The picks are read where the device has them:
  // the greedy tail's argmax leaves a second copy of its ids in lp_picks
  // (launch_argmax's ids2); the sampling kernel has one ids output, the pinned
  // results, so under do_sample the combine launch reads each row's pick from
  // there (4 bytes per row over PCIe, once).
  bool logprobs = false;
  float *lp_h = nullptr;        // [Tm], pinned
  int32_t *lp_picks = nullptr;  // [Tm]
  char *lp_ws = nullptr;
  size_t lp_ws_bytes = 0;
  StepExtra<int32_t> step_targets;
  bool logprobs_on() const override { return logprobs; }
  ffmi_status set_logprobs(bool on) override {
    const char *why = mode == FFMI_MODEL_BEAM
                          ? "logprobs: a BEAM model's picks are proposals, not tokens"
                          : Vl != c.vocab_size ? "logprobs: vocab-sharded lm_head" : nullptr;
    if (why) return refuse(why);
    if (on && !lp_ws) {
      FFMI_CHECK(Vl <= ffmi::sample_topp_max_v(), FFMI_ERR_UNSUPPORTED);
      if (!lp_h)
        FFMI_HIP(hipHostMalloc((void **)&lp_h, Tm * sizeof(float),
                               hipHostMallocCoherent | hipHostMallocMapped));
      ffmi_status st = lp_picks ? FFMI_OK : alloc(&lp_picks, Tm);
      if (st != FFMI_OK) return st;
      lp_ws_bytes = ffmi::token_logprobs_workspace_bytes(Tm, Vl);
      if ((st = alloc(&lp_ws, lp_ws_bytes)) != FFMI_OK) return st;
    }
    // (the captured graphs hold the step with or without the launches)
    FFMI_HIP(hipStreamSynchronize(stream));
    clear_graphs();
    logprobs = on;
    return FFMI_OK;
  }
  // the step's targets, from the batch the scheduler built
  void take_step_targets(const BatchConfig &bc) {
    step_targets.v.resize(bc.num_tokens);
    for (int t = 0; t < bc.num_tokens; ++t) step_targets.v[t] = bc.tokensInfo[t].score_id;
  }
  // LoRA adapters (FFMI_MODEL_LORA; lora_linear.cc) on q / k / v / o and
  // down_proj.  Each row's adapter (BatchConfig::PerRequestInfo::lora_id of
  // its request, -1 for an adapter this model did not load) rides the blob
  // behind the records, the draws and the targets, so a replayed graph reads
  // fresh assignments.  The step's module mask -- the union of the modules of
  // the adapters its rows name -- decides which sites leave their fused route
  // and run the LoRA launches (enqueue), and is part of the graph key.  On a
  // model that uses the fused residual norms, which are not bit-identical to
  // the norm launches, the modules of every resident adapter with an
  // attention module count too (lora_route), so that a row without an adapter
  // has the same bits in every step.  Adapter storage and the device table
  // [L][kLoraMods][FFMI_LORA_MAX_ADAPTERS] are allocated at creation / load,
  // never in a step.
  static constexpr int kLoraMods = 5;  // FFMI_LORA_Q .. FFMI_LORA_DOWN
  static constexpr unsigned kLoraQKV = FFMI_LORA_Q_BIT | FFMI_LORA_K_BIT | FFMI_LORA_V_BIT;
  bool lora = false;
  ffmi_lora_entry *lora_tab = nullptr;
  std::vector<ffmi_lora_entry> lora_tab_h;
  uint16_t *lora_A[kLoraMods][FFMI_LORA_MAX_ADAPTERS] = {}, *lora_B[kLoraMods][FFMI_LORA_MAX_ADAPTERS] = {};
  unsigned lora_mods[FFMI_LORA_MAX_ADAPTERS] = {};  // modules of each loaded adapter (0: not loaded)
  float *lora_ws = nullptr;
  StepExtra<int32_t> step_slots;
  unsigned step_lora_mask = 0;
  size_t lora_tab_at(int l, int mod, int id) const {
    return ((size_t)l * kLoraMods + mod) * FFMI_LORA_MAX_ADAPTERS + id;
  }
  // (the step-independent part of enqueue's `fuse`: can any step of this model
  // take the fused residual norms?)
  bool lora_fuse_capable() const {
    return (fuse_norms == 2 || (fuse_norms == 1 && c.hidden >= 2048)) && o.tp_size == 1 &&
           c.hidden % 32 == 0 && Hl % 32 == 0 && c.hidden <= 4096;
  }
  void take_step_slots(const BatchConfig &bc) {
    step_slots.v.resize(bc.num_tokens);
    step_lora_mask = 0;
    for (int t = 0; t < bc.num_tokens; ++t) {
      const int a = bc.requestsInfo[bc.tokensInfo[t].request_index].lora_id;
      step_slots.v[t] = a >= 0 && a < FFMI_LORA_MAX_ADAPTERS && lora_mods[a] ? a : -1;
      if (step_slots.v[t] >= 0) step_lora_mask |= lora_mods[a];
    }
  }
  // the modules whose route this step takes
  unsigned lora_route() const {
    if (!lora) return 0;
    unsigned m = step_lora_mask;
    // (a down-only adapter keeps the per-step route it has always had: a step
    // that names none is the fused step, launch for launch)
    if (lora_fuse_capable())
      for (int a = 0; a < FFMI_LORA_MAX_ADAPTERS; ++a)
        if (lora_mods[a] & ~FFMI_LORA_DOWN_BIT) m |= lora_mods[a];
    return m;
  }
  static ffmi_status refuse(const char *why) {
    ffmi_set_last_error(why, __FILE__, __LINE__);
    return FFMI_ERR_UNSUPPORTED;
  }
  static ffmi_status invalid(const char *why) {
    ffmi_set_last_error(why, __FILE__, __LINE__);
    return FFMI_ERR_INVALID;
  }
  // a module's dimensions: the HF tensor's (in, out) and the device's out
  // (k / v under the replicated load: every query head its K/V head's rows)
  void lora_dims(int mod, int *in, int *out_hf, int *out_dev) const {
    const int H = c.hidden;
    *in = mod == FFMI_LORA_DOWN ? Fl : H;
    const bool kv = mod == FFMI_LORA_K || mod == FFMI_LORA_V;
    *out_hf = kv ? c.num_kv_heads * d : H;
    *out_dev = kv ? Hkv : mod == FFMI_LORA_Q ? Hl : H;
  }
  ffmi_status lora_load(int rank, float alpha, const void *A, const void *B, int *id_out) override {
    if (!lora) return ffmi_model::lora_load(rank, alpha, A, B, id_out);
    FFMI_CHECK(A && B && id_out && rank >= 1 && std::isfinite(alpha), FFMI_ERR_INVALID);
    const ffmi_lora_module m{FFMI_LORA_DOWN, A, B};
    return lora_load_modules(rank, alpha, 1, &m, id_out);
  }
  ffmi_status lora_load_modules(int rank, float alpha, int n, const ffmi_lora_module *mods,
                                int *id_out) override {
    if (!lora) return ffmi_model::lora_load_modules(rank, alpha, n, mods, id_out);
    if (n <= 0 || !mods) return invalid("lora: an adapter without modules");
    unsigned seen = 0;
    for (int i = 0; i < n; ++i) {
      const int mod = mods[i].module;
      if (mod == FFMI_LORA_GATE || mod == FFMI_LORA_UP)
        return refuse("lora: gate_proj / up_proj adapters are not served");
      if (mod < 0 || mod >= kLoraMods) return invalid("lora: unknown module");
      if ((seen >> mod) & 1u) return invalid("lora: a module listed twice");
      seen |= 1u << mod;
    }
    FFMI_CHECK(id_out && rank >= 1 && std::isfinite(alpha), FFMI_ERR_INVALID);
    for (int i = 0; i < n; ++i) FFMI_CHECK(mods[i].A && mods[i].B, FFMI_ERR_INVALID);
    if (rank > FFMI_LORA_MAX_RANK) return refuse("lora: rank above FFMI_LORA_MAX_RANK");
    const int L = c.num_layers, R = FFMI_LORA_MAX_RANK;
    const int id = lora_id_acquire(this);
    if (id < 0) {
      ffmi_set_last_error("lora: FFMI_LORA_MAX_ADAPTERS adapters are loaded", __FILE__, __LINE__);
      return FFMI_ERR_OOM;
    }
    const _Float16 s16 = (_Float16)(alpha / (float)rank);
    const hipError_t e0 = hipStreamSynchronize(stream);
    bool oom = false, bad = e0 != hipSuccess;
    for (int i = 0; i < n && !oom && !bad; ++i) {
      const int mod = mods[i].module;
      int F, No, N;
      lora_dims(mod, &F, &No, &N);
      // A as the packed activation tiles of a [R][F] matrix (one MFMA operand
      // fragment per 16 ranks x 32 columns), B [N][R]; zero beyond the rank
      const uint16_t *a = static_cast<const uint16_t *>(mods[i].A);
      const uint16_t *b = static_cast<const uint16_t *>(mods[i].B);
      const int G = N / No;  // (> 1: k / v rows replicated to the query heads)
      std::vector<uint16_t> ap((size_t)L * R * F, 0), bp((size_t)L * N * R, 0);
      for (int l = 0; l < L; ++l) {
        for (int j = 0; j < rank; ++j)
          for (int k = 0; k < F; ++k)
            ap[(size_t)l * R * F + act_packed_off(j, k, F)] = a[((size_t)l * rank + j) * F + k];
        for (int r = 0; r < N; ++r) {
          const int src = G > 1 ? (r / d / G) * d + r % d : r;
          memcpy(&bp[((size_t)l * N + r) * R], &b[((size_t)l * No + src) * rank], (size_t)rank * 2);
        }
      }
      uint16_t *ad = nullptr, *bd = nullptr;
      if (hipMalloc((void **)&ad, ap.size() * 2) != hipSuccess ||
          hipMalloc((void **)&bd, bp.size() * 2) != hipSuccess) {
        (void)hipFree(ad);
        (void)hipGetLastError();
        oom = true;
        break;
      }
      lora_A[mod][id] = ad, lora_B[mod][id] = bd;
      for (int l = 0; l < L; ++l) {
        ffmi_lora_entry &e = lora_tab_h[lora_tab_at(l, mod, id)];
        e.A = ad + (size_t)l * R * F, e.B = bd + (size_t)l * N * R;
        e.scale = (float)s16, e.rank = rank;
      }
      // (blocking copies; steps in flight read the table's other entries only)
      bad = hipMemcpy(ad, ap.data(), ap.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(bd, bp.data(), bp.size() * 2, hipMemcpyHostToDevice) != hipSuccess;
    }
    if (!oom && !bad)
      bad = hipMemcpy(lora_tab, lora_tab_h.data(), lora_tab_h.size() * sizeof(ffmi_lora_entry),
                      hipMemcpyHostToDevice) != hipSuccess;
    if (oom || bad) {
      (void)hipGetLastError();
      (void)lora_unload(id);
      ffmi_set_last_error(oom ? "lora: adapter alloc" : "lora: adapter upload", __FILE__, __LINE__);
      return oom ? FFMI_ERR_OOM : FFMI_ERR_HIP;
    }
    lora_mods[id] = seen;
    *id_out = id;
    return FFMI_OK;
  }
  // one per-tensor file of the reference's adapter folder
  ffmi_status lora_read(const std::string &path, size_t n, uint16_t *dst) {
    return tensor_status(read_tensor(path, n, dst), "lora: adapter file", path);
  }
  // (the older entry point keeps tensor_status's own code for a missing or
  // wrong-sized file; _ex answers FFMI_ERR_UNSUPPORTED, as its contract says)
  ffmi_status lora_load_folder(const char *folder, int rank, float alpha, int *id_out) override {
    if (!lora) return ffmi_model::lora_load_folder(folder, rank, alpha, id_out);
    return lora_load_files(folder, rank, alpha, FFMI_LORA_DOWN_BIT, id_out, false);
  }
  ffmi_status lora_load_folder_ex(const char *folder, int rank, float alpha, unsigned modules,
                                  int *id_out) override {
    if (!lora) return ffmi_model::lora_load_folder_ex(folder, rank, alpha, modules, id_out);
    return lora_load_files(folder, rank, alpha, modules, id_out, true);
  }
  ffmi_status lora_load_files(const char *folder, int rank, float alpha, unsigned modules,
                              int *id_out, bool file_unsupported) {
    FFMI_CHECK(rank >= 1, FFMI_ERR_INVALID);
    if (rank > FFMI_LORA_MAX_RANK) return refuse("lora: rank above FFMI_LORA_MAX_RANK");
    if (modules & ((1u << FFMI_LORA_GATE) | (1u << FFMI_LORA_UP)))
      return refuse("lora: gate_proj / up_proj adapters are not served");
    if (!modules || (modules >> kLoraMods)) return invalid("lora: no module, or an unknown one, in the mask");
    static const char *const names[kLoraMods] = {".self_attn.q_proj.lora_", ".self_attn.k_proj.lora_",
                                                 ".self_attn.v_proj.lora_", ".self_attn.o_proj.lora_",
                                                 ".mlp.down_proj.lora_"};
    // an adapter tensor of a module outside the mask (gate / up included) refuses
    if (DIR *dir = opendir(folder)) {
      bool other = false;
      while (const dirent *de = readdir(dir)) {
        const std::string n = de->d_name;
        if (n.find(".lora_") == std::string::npos) continue;
        bool mine = false;
        for (int mod = 0; mod < kLoraMods; ++mod)
          mine = mine || (((modules >> mod) & 1u) && n.find(names[mod]) != std::string::npos);
        other = other || !mine;
      }
      closedir(dir);
      if (other) return refuse("lora: the folder holds an adapter tensor of a module that was not asked for");
    }
    const int L = c.num_layers;
    std::vector<std::vector<uint16_t>> as, bs;
    std::vector<ffmi_lora_module> mods;
    for (int mod = 0; mod < kLoraMods; ++mod) {
      if (!((modules >> mod) & 1u)) continue;
      int F, No, N;
      lora_dims(mod, &F, &No, &N);
      // (the files hold the unsharded HF tensors; tp_size is 1 under the flag)
      as.emplace_back((size_t)L * rank * F), bs.emplace_back((size_t)L * No * rank);
      for (int l = 0; l < L; ++l) {
        const std::string p = std::string(folder) + "/layers." + std::to_string(l) + names[mod];
        ffmi_status st = lora_read(p + "A.weight", (size_t)rank * F, &as.back()[(size_t)l * rank * F]);
        if (st == FFMI_OK) st = lora_read(p + "B.weight", (size_t)No * rank, &bs.back()[(size_t)l * No * rank]);
        if (st != FFMI_OK) return file_unsupported ? FFMI_ERR_UNSUPPORTED : st;
      }
    }
    for (int mod = 0, i = 0; mod < kLoraMods; ++mod)
      if ((modules >> mod) & 1u) {
        mods.push_back(ffmi_lora_module{mod, as[i].data(), bs[i].data()});
        ++i;
      }
    return lora_load_modules(rank, alpha, (int)mods.size(), mods.data(), id_out);
  }
  void lora_free(int id) {
    for (int mod = 0; mod < kLoraMods; ++mod) {
      (void)hipFree(lora_A[mod][id]), (void)hipFree(lora_B[mod][id]);
      lora_A[mod][id] = lora_B[mod][id] = nullptr;
    }
    lora_mods[id] = 0;
  }
  ffmi_status lora_unload(int id) override {
    if (!lora) return ffmi_model::lora_unload(id);
    if (!lora_id_release(this, id)) {
      ffmi_set_last_error("lora: not this model's adapter, or a registered request names it",
                          __FILE__, __LINE__);
      return FFMI_ERR_INVALID;
    }
    // no step reads the entries any more: clear them, then free the storage
    for (int l = 0; l < c.num_layers; ++l)
      for (int mod = 0; mod < kLoraMods; ++mod) lora_tab_h[lora_tab_at(l, mod, id)] = ffmi_lora_entry{};
    const hipError_t e0 = hipStreamSynchronize(stream);
    const hipError_t e1 = hipMemcpy(lora_tab, lora_tab_h.data(),
                                    lora_tab_h.size() * sizeof(ffmi_lora_entry), hipMemcpyHostToDevice);
    lora_free(id);
    FFMI_HIP(e0);
    FFMI_HIP(e1);
    return FFMI_OK;
  }
  // vocab-sharded lm_head at TP > 1 (model.cc:3392-3419): this rank's Vl rows
  // and the [P][Tm][kXW] exchange records of the sharded softmax / top-k
  int Vl = 0;
  float *xch = nullptr;
  // TP over the direct xGMI transport (ffmi_comm_peer_attach): the
  // row-parallel GEMMs run in two column halves; each half is all-reduced on
  // comm_stream while the next half computes (allreduce.cc:291-331 runs the
  // collective as a concurrent task; here it overlaps on HIP streams)
  bool peer = false;
  // RCCL all-reduce (no transport attached, or the transport cannot hold a
  // step): the same two-half overlap and graph capture as over the transport
  // (ncclAllReduce is stream-capturable); an in-process local group is not
  // (its all-reduce synchronises the host) and runs eager and unsplit
  bool rccl = false;
  bool solo = false;  // TP shard over a 1-rank communicator without transport or RCCL
  // residual norms folded into the skinny GEMMs around them (T <= 32, TP = 1):
  // per-tile sums of squares of the residual after o (ss_o) and after down
  // (ss_d), [32][H/16] each.  Only where o/down run unsplit anyway (H/16 >=
  // 128 tiles: LLaMA-7B decode, +1.9% incr decoding -- the A/B of record is
  // profiles/r03_fused_norm_ab.log, quoted in DESIGN.md §5); the 68M SSM's
  // o/down split K over workgroups, and unsplitting them to fuse cost more
  // than the norm launches saved (SSM step +4 us).  FFMI_FUSE_NORM: 0 off,
  // 1 auto (default), 2 every width (tests)
  int fuse_norms = getenv("FFMI_FUSE_NORM") ? atoi(getenv("FFMI_FUSE_NORM")) : 1;
  float *ss_o = nullptr, *ss_d = nullptr;
  // output projection folded into the fused attention (ffmi::OprojArgs): a
  // small model (d = 64, H <= 1024 -- the 68M SSM) at TP = 1 skips its o_proj
  // launch; the attention leaves one fp32 slab per head [heads][T][H] for the
  // residual norm.  FFMI_FUSE_AO=0 turns it off (A/B, tests)
  bool fuse_ao = false;
  float *oslab = nullptr;
  int oslab_T = 0;
  // the residual norm after each all-reduce folded into it over the transport
  // (ffmi::comm_allreduce_norm; the reference's AllReduce -> ResidualRMSNorm,
  // model.cc:3421-3445): no norm launch per all-reduce, and in two-shot mode
  // each rank normalises only its T / N rows (res is then current on those
  // rows only; h is complete).  FFMI_TP_FUSED_NORM: 0 off, 1 on (not with
  // debug captures), 2 also with debug captures (tests: the h and logits
  // captures are then of the fused path; o_proj / down / hidden are not kept)
  int tp_fuse_norm = getenv("FFMI_TP_FUSED_NORM") ? atoi(getenv("FFMI_TP_FUSED_NORM")) : 1;
  int tp_chunks = 1;
  hipStream_t comm_stream = nullptr;
  uint16_t *chunk_buf = nullptr;  // [tp_chunks][Tm][H / tp_chunks]
  std::vector<hipEvent_t> ev_chunk;
  hipEvent_t ev_comm_done = nullptr;
  float *ws = nullptr;  // split-K workspace of the GEMMs
  size_t ws_bytes = 0;
  size_t ws_chunk = 0;  // per-chunk workspace of the overlapped row-parallel GEMMs
  // split-K slabs summed by the all-reduce's copy-in (FFMI_AR_SLABS=0: the
  // GEMM's own reduce pass, A/B runs)
  bool ar_slabs = !getenv("FFMI_AR_SLABS") || atoi(getenv("FFMI_AR_SLABS")) != 0;
  int32_t *ids_h = nullptr;  // [kChain slots][Tm * 4 ids | Tm * 4 probs], pinned
  // chained beam steps (beam_launch_chained): one staging blob and one result
  // slot per step of a speculation phase; the top-k also leaves each slot's
  // ids in device memory (ids_dev) for the next step's embedding gather.
  // Slot 0 is also every unchained step's; the others exist only in a BEAM
  // model at TP = 1 (init), the only one that chains (can_chain_beam)
  static constexpr int kChain = BeamSearchBatchConfig::MAX_BEAM_DEPTH;
  ffmi_batch_dev *chain_batch[kChain] = {};
  int32_t *ids_dev = nullptr;  // [kChain][Tm * 4]
  size_t slot_results[kChain] = {};  // [T][k] ids of each slot
  std::vector<int> slot_map[kChain];  // scheduler entry -> [T][k] index (beam_result_layout)
  hipEvent_t slot_ev[kChain] = {};     // recorded behind each launched slot
  hipEvent_t chain_t0 = nullptr;       // (FFMI_STEP_TIMING: before a chain's slot 0)
  bool slot_ev_live[kChain] = {};      // slot_ev recorded for the chain in flight
  int last_slot = -1;                  // highest slot launched since the last wait
  bool chain_ok = !getenv("FFMI_SSM_CHAIN") || atoi(getenv("FFMI_SSM_CHAIN")) != 0;
  size_t slot_ints() const { return (size_t)Tm * 4 * 2; }
  int32_t *slot_ids_h(int slot) const { return ids_h + slot * slot_ints(); }
  int32_t *slot_ids_dev(int slot) const { return ids_dev + (size_t)slot * (slot_ints() / 2); }
  bool result_copy = getenv("FFMI_RESULT_COPY") && atoi(getenv("FFMI_RESULT_COPY")) != 0;
  PackedStep ps;
  std::vector<void *> allocs;

  // ---- per-op profiling (HIP events on `stream`) ----
  enum Cat { GEMM_QKV, GEMM_O, GEMM_GATE_UP, GEMM_DOWN, GEMM_LM_HEAD, ATTENTION, NORM,
             ALLREDUCE, SAMPLING, EMBED, LOGPROBS, LORA, NCAT };
  struct ProfRec {
    int cat;
    hipEvent_t a, b;
    double bytes, flops;
  };
  struct OpStat {
    long launches = 0;
    double ms = 0, bytes = 0, flops = 0;
  };
  int prof_level = 0;
  // level 1 samples every prof_every-th step (FFMI_PROF_EVERY, default 4):
  // event-bracketed steps run eager, and bracketing every step cost the
  // bench ~2.5 % of its tokens/s
  int prof_every = getenv("FFMI_PROF_EVERY") ? std::max(1, atoi(getenv("FFMI_PROF_EVERY"))) : 4;
  long prof_steps = 0;
  bool prof_this_step = true;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<ProfRec> recs;
  OpStat opstat[NCAT];

  hipEvent_t next_event() {
    if (ev_used == ev_pool.size()) {
      hipEvent_t e;
      (void)hipEventCreate(&e);
      ev_pool.push_back(e);
    }
    return ev_pool[ev_used++];
  }
  bool prof_on(int layer, int T) const {
    if (prof_level == 2) return true;
    if (prof_level == 1)
      return prof_this_step && T <= 256 && (layer == 0 || layer == c.num_layers / 2);
    return false;
  }
  int prof_begin(bool on) {
    if (!on) return -1;
    ProfRec r;
    r.a = next_event();
    r.b = next_event();
    (void)hipEventRecord(r.a, stream);
    recs.push_back(r);
    return (int)recs.size() - 1;
  }
  void prof_end(int idx, int cat, double bytes, double flops) {
    if (idx < 0) return;
    ProfRec &r = recs[idx];
    r.cat = cat;
    r.bytes = bytes;
    r.flops = flops;
    (void)hipEventRecord(r.b, stream);
  }
  void prof_collect() {
    for (auto &r : recs) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
      OpStat &o = opstat[r.cat];
      o.launches++;
      o.ms += ms;
      o.bytes += r.bytes;
      o.flops += r.flops;
    }
    recs.clear();
    ev_used = 0;
  }
  ffmi_status set_profiling(int level) override {
    prof_level = level;
    prof_steps = 0;
    for (auto &o : opstat) o = OpStat();
    return FFMI_OK;
  }
  int op_stats(ffmi_op_stat *out, int cap) override {
    static const char *names[NCAT] = {"gemm_qkv", "gemm_o_proj", "gemm_gate_up_silu",
                                      "gemm_down", "gemm_lm_head", "attention", "rmsnorm",
                                      "rowpar_gemm_allreduce", "softmax_argmax", "embedding",
                                      "token_logprobs", "lora"};
    int n = 0;
    for (int i = 0; i < NCAT; ++i) {
      if (opstat[i].launches == 0) continue;
      if (out && n < cap) {
        snprintf(out[n].name, sizeof(out[n].name), "%s", names[i]);
        out[n].launches = opstat[i].launches;
        out[n].total_ms = opstat[i].ms;
        out[n].bytes = opstat[i].bytes;
        out[n].flops = opstat[i].flops;
      }
      ++n;
    }
    return n;
  }
  static double gemm_bytes(int T, int N_w, int N_out, int K) {
    return 2.0 * ((double)N_w * K + (double)T * K + (double)T * N_out);
  }
  double attn_bytes() const {
    // K and V of every visible slot of each request read once + qkv in + out
    std::vector<int> kv(o.max_requests, 0);
    for (const auto &w : ps.work) kv[w.req] = std::max(kv[w.req], w.kv_len);
    double b = 0;
    for (int r : kv) b += (double)r * Hkv * 2 * 2;
    return b + (double)ps.tokens.size() * (Nqkv + Hl) * 2;
  }

  // ---- tensor capture (--inference-debugging, operator.h:271-360) ----
  // kind k (FFMI_DBG_*) keeps [dbg_layers(k)][Tm][dbg_width(k)] fp16 values of
  // the last eager step; GEMM inputs are stored in their packed tile layout
  // and unpacked on readout
  static constexpr int kDbgKinds = 10;
  int dbg = 0;
  uint16_t *dbg_buf = nullptr;
  size_t dbg_off[kDbgKinds] = {};
  int dbg_T = -1;
  size_t kv_cache_bytes() const override {
    size_t b = 0;
    for (const auto &L : layers) b += ffmi_attn_cache_bytes(L.attn);
    return b;
  }
  long debug_width(int k) const override {
    switch (k) {
      case FFMI_DBG_LOGITS: return Vl;
      case FFMI_DBG_QKV: return Nqkv;
      case FFMI_DBG_ATTN_OUT: return Hl;
      case FFMI_DBG_MLP_ACT: return Fl;
      case FFMI_DBG_HIDDEN: case FFMI_DBG_ATTN_NORM: case FFMI_DBG_O_PROJ:
      case FFMI_DBG_FFN_NORM: case FFMI_DBG_DOWN: case FFMI_DBG_EMBED: return c.hidden;
    }
    return -1;
  }
  int dbg_layers(int k) const {
    return k == FFMI_DBG_LOGITS ? 0 : k == FFMI_DBG_EMBED ? 1
                                    : k == FFMI_DBG_HIDDEN ? c.num_layers + 1 : c.num_layers;
  }
  // stored in the packed activation-tile layout (a GEMM input written so)
  bool dbg_is_packed(int k, int layer) const {
    if (!packed) return false;
    return k == FFMI_DBG_ATTN_NORM || k == FFMI_DBG_FFN_NORM || k == FFMI_DBG_ATTN_OUT ||
           k == FFMI_DBG_MLP_ACT || (k == FFMI_DBG_HIDDEN && layer == c.num_layers);
  }
  static int rows16(int T) { return (T + 15) / 16 * 16; }  // rows of T's packed tiles
  ffmi_status set_debug(int enable) override {
    if (enable && !dbg_buf) {
      size_t total = 0;
      for (int k = 0; k < kDbgKinds; ++k) {
        dbg_off[k] = total;
        total += (size_t)dbg_layers(k) * Tm * std::max(0L, debug_width(k));
      }
      if (alloc(&dbg_buf, total) != FFMI_OK) return FFMI_ERR_OOM;
    }
    dbg = enable ? 1 : 0;
    dbg_T = -1;
    return FFMI_OK;
  }
  uint16_t *dbg_slot(int k, int l) const {
    return dbg_buf + dbg_off[k] + (size_t)l * Tm * debug_width(k);
  }
  // capture src ([T][width], or packed tiles covering whole 16-row groups)
  ffmi_status dbg_copy(int k, int l, const uint16_t *src, int T) {
    const size_t rows = (size_t)(dbg_is_packed(k, l) ? rows16(T) : T);
    FFMI_HIP(hipMemcpyAsync(dbg_slot(k, l), src, rows * debug_width(k) * 2,
                            hipMemcpyDeviceToDevice, stream));
    return FFMI_OK;
  }
  // capture a GEMM output that is either written (Y) or left as split-K slabs
  ffmi_status dbg_gemm_out(int k, int l, const uint16_t *Y, const ffmi::Partials &p, int T) {
    if (p.S > 0) {
      FFMI_HIP(ffmi::launch_partials_reduce(p, dbg_slot(k, l), T, (int)debug_width(k), stream));
      return FFMI_OK;
    }
    return dbg_copy(k, l, Y, T);
  }
  long debug_tensor(int which, int layer, float *out, long cap) override {
    if (dbg_T < 0 || (stream && hipStreamSynchronize(stream) != hipSuccess)) return -1;
    if (which < 0 || which >= kDbgKinds) return -1;
    const int T = dbg_T;
    const long width = debug_width(which);
    if (which != FFMI_DBG_LOGITS && (layer < 0 || layer >= dbg_layers(which))) return -1;
    if (cap < (long)T * width) return -1;
    const uint16_t *src = which == FFMI_DBG_LOGITS ? logits : dbg_slot(which, layer);
    const bool pk = which != FFMI_DBG_LOGITS && dbg_is_packed(which, layer);
    const size_t n = (size_t)(pk ? rows16(T) : T) * width;
    std::vector<uint16_t> raw(n);
    if (hipMemcpy(raw.data(), src, n * 2, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (int t = 0; t < T; ++t)
      for (long j = 0; j < width; ++j) {
        const uint16_t b = raw[pk ? act_packed_off(t, (int)j, (int)width) : (size_t)t * width + j];
        _Float16 v;
        memcpy(&v, &b, 2);
        out[(size_t)t * width + j] = (float)v;
      }
    return T;
  }

  // FFMI_FAULT_TP_AR_DROP: this rank's contribution to one all-reduce zeroed
  int ar_drop_layer = -1, ar_drop_which = 0;
  bool ar_drop_now = false;  // (set around the faulted call in enqueue)
  std::vector<int> head_swapped;  // layers whose Q heads 0 / 1 are exchanged

  // pack the Q rows of layer l with local heads 0 and 1 exchanged (swap) or
  // in their places; the source rows are regenerated / reloaded
  ffmi_status pack_q_heads(int l, bool swap) {
    const int H = c.hidden, s = o.tp_rank;
    uint16_t *tmp = nullptr;
    FFMI_HIP(hipMalloc((void **)&tmp, (size_t)H * H * 2));
    const std::string p = "model.layers." + std::to_string(l) + ".self_attn.q_proj.weight";
    ffmi_status st = FFMI_OK;
    if (!weights_folder.empty()) {
      st = load_tensor(tmp, (size_t)H * H, p);
    } else if (launch_fill_weight(tmp, (size_t)H * H, ffmi::weight_key(p.c_str(), o.weight_seed),
                                  0, stream) != hipSuccess) {
      st = FFMI_ERR_HIP;
    }
    if (st == FFMI_OK) {
      const int pitch = Nqkv / 16;
      const hipError_t e0 = launch_pack_weight(tmp, H, s * Hl + (swap ? d : 0), 0, d, H,
                                               layers[l].wqkv, 1, 0, pitch, stream);
      const hipError_t e1 = launch_pack_weight(tmp, H, s * Hl + (swap ? 0 : d), 0, d, H,
                                               layers[l].wqkv, 1, d / 16, pitch, stream);
      if (e0 != hipSuccess || e1 != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
        st = FFMI_ERR_HIP;
    }
    (void)hipFree(tmp);
    return st;
  }

  ffmi_status debug_fault(int kind, int layer, int arg) override {
    // the tables are rewritten with blocking copies: finish the model's
    // (non-blocking) stream first in every branch
    if (stream) FFMI_HIP(hipStreamSynchronize(stream));
    if (kind == FFMI_FAULT_TP_HEAD_SWAP) {
      FFMI_CHECK(layer >= -1 && layer < c.num_layers && heads_l >= 2 && d % 16 == 0,
                 FFMI_ERR_INVALID);
      for (int l = 0; l < c.num_layers; ++l)
        if ((layer < 0 || l == layer) &&
            std::find(head_swapped.begin(), head_swapped.end(), l) == head_swapped.end()) {
          ffmi_status st = pack_q_heads(l, true);
          if (st != FFMI_OK) return st;
          head_swapped.push_back(l);
        }
      clear_graphs();
      return FFMI_OK;
    }
    if (kind == FFMI_FAULT_TP_AR_DROP) {
      FFMI_CHECK(o.tp_size > 1 && layer >= 0 && layer < c.num_layers && (arg == 0 || arg == 1),
                 FFMI_ERR_INVALID);
      ar_drop_layer = layer;
      ar_drop_which = arg;
      clear_graphs();
      return FFMI_OK;
    }
    if (kind == FFMI_FAULT_NONE) {
      for (int l : head_swapped) {
        ffmi_status st = pack_q_heads(l, false);
        if (st != FFMI_OK) return st;
      }
      head_swapped.clear();
      ar_drop_layer = -1;
      clear_graphs();
    }
    if (kind == FFMI_FAULT_RESID_ROUND || kind == FFMI_FAULT_NONE) {
      // captured graphs hold the launches of the other norm variant
      ffmi::set_norm_fault(kind == FFMI_FAULT_RESID_ROUND);
      clear_graphs();
      if (kind == FFMI_FAULT_RESID_ROUND) return FFMI_OK;
    }
    if (kind == FFMI_FAULT_NONE) {
      for (auto &L : layers) {
        ffmi_status st = ffmi::attn_rope_fault(L.attn, -1);
        if (st != FFMI_OK) return st;
      }
      return FFMI_OK;
    }
    FFMI_CHECK(kind == FFMI_FAULT_ROPE_POS && layer >= -1 && layer < c.num_layers,
               FFMI_ERR_INVALID);
    for (int l = 0; l < c.num_layers; ++l)
      if (layer < 0 || l == layer) {
        ffmi_status st = ffmi::attn_rope_fault(layers[l].attn, arg);
        if (st != FFMI_OK) return st;
      }
    return FFMI_OK;
  }

  ~LlamaGPU() override {
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto &kv : st_sum) {
      if (kv.first < 0) {
        fprintf(stderr, "[ffmi step timing] H=%d chain of %d steps: %ld chains, gpu span %.1f us "
                "(%.1f us per step)\n", c.hidden, -kv.first, kv.second.n,
                kv.second.gpu / kv.second.n, kv.second.gpu / kv.second.n / -kv.first);
        continue;
      }
      fprintf(stderr, "[ffmi step timing] H=%d T=%d steps=%ld launch=%.1f gpu=%.1f wait=%.1f total=%.1f us\n",
              c.hidden, kv.first, kv.second.n, kv.second.launch / kv.second.n, kv.second.gpu / kv.second.n,
              kv.second.wait / kv.second.n, kv.second.total / kv.second.n);
    }
    for (auto e : st_ev)
      if (e) (void)hipEventDestroy(e);
    for (auto e : slot_ev)
      if (e) (void)hipEventDestroy(e);
    if (chain_t0) (void)hipEventDestroy(chain_t0);
    clear_graphs();
    lora_id_release_all(this);
    for (int i = 0; i < FFMI_LORA_MAX_ADAPTERS; ++i) lora_free(i);
    for (auto &L : layers) ffmi_attn_destroy(L.attn);
    for (auto e : ev_pool) (void)hipEventDestroy(e);
    for (auto e : ev_chunk) (void)hipEventDestroy(e);
    if (ev_comm_done) (void)hipEventDestroy(ev_comm_done);
    if (comm_stream) (void)hipStreamDestroy(comm_stream);
    for (void *p : allocs) (void)hipFree(p);
    if (ids_h) (void)hipHostFree(ids_h);
    if (lp_h) (void)hipHostFree(lp_h);
    for (ffmi_batch_dev *b : chain_batch) ffmi_batch_destroy(b);
    if (stream) (void)hipStreamDestroy(stream);
  }

  template <typename T>
  ffmi_status alloc(T **p, size_t elems) {
    if (hipMalloc((void **)p, elems * sizeof(T)) != hipSuccess) {
      ffmi_set_last_error("model alloc", __FILE__, __LINE__);
      return FFMI_ERR_OOM;
    }
    allocs.push_back(*p);
    return FFMI_OK;
  }

  // One tensor of a reference-format checkpoint (tensor_file.h); a GQA
  // checkpoint's K/V replicated per query head unless native_gqa keeps them
  ffmi_status load_tensor(uint16_t *dst, size_t n, const std::string &hf_name) {
    std::vector<uint16_t> h16;
    std::string path;
    const TensorRead r = read_checkpoint_tensor(weights_folder, hf_name, n, c.num_heads,
                                                native_gqa ? c.num_heads : c.num_kv_heads, &h16, &path);
    if (r != TensorRead::ok) return tensor_status(r, "weight file", path);
    FFMI_HIP(hipMemcpy(dst, h16.data(), n * 2, hipMemcpyHostToDevice));
    return FFMI_OK;
  }

  ffmi_status init() {
    const int H = c.hidden, F = c.intermediate, V = c.vocab_size, P = o.tp_size;
    // GQA checkpoints load with K/V replicated per query head (the
    // reference's layout) and synthetic weights are MHA only -- unless the
    // model was created with FFMI_MODEL_NATIVE_GQA: K/V at num_kv_heads, from
    // a checkpoint or the generator, each rank its own K/V heads
    native_gqa = native_gqa && c.num_kv_heads != c.num_heads;
    FFMI_CHECK(c.num_kv_heads == c.num_heads ||
                   ((native_gqa || !weights_folder.empty()) && c.num_kv_heads > 0 &&
                    c.num_heads % c.num_kv_heads == 0),
               FFMI_ERR_UNSUPPORTED);
    FFMI_CHECK(H % c.num_heads == 0 && c.num_heads % P == 0 && F % P == 0, FFMI_ERR_INVALID);
    if (native_gqa && c.num_kv_heads % P != 0) {
      ffmi_set_last_error("native_gqa: num_kv_heads is not a multiple of tp_size (the replicated "
                          "load takes this case)", __FILE__, __LINE__);
      return FFMI_ERR_UNSUPPORTED;
    }
    d = H / c.num_heads;
    // (d = 32: incremental decoding only, as the reference's kernels)
    FFMI_CHECK(d == 64 || d == 128 || (d == 32 && mode == FFMI_MODEL_INC), FFMI_ERR_UNSUPPORTED);
    heads_l = c.num_heads / P;
    Hl = heads_l * d;
    kvh_l = native_gqa ? c.num_kv_heads / P : heads_l;
    Hkv = kvh_l * d;
    Nqkv = Hl + 2 * Hkv;
    if (native_gqa && d != 64 && d != 128) {
      ffmi_set_last_error("native_gqa: head_dim 64 or 128", __FILE__, __LINE__);
      return FFMI_ERR_UNSUPPORTED;
    }
    Fl = F / P;
    FFMI_CHECK(H % 32 == 0 && Hl % 32 == 0 && Fl % 32 == 0, FFMI_ERR_UNSUPPORTED);
    FFMI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    Tm = (o.max_tokens + 15) & ~15;
    packed = H % 32 == 0 && Hl % 32 == 0 && Fl % 32 == 0;
    {
      const double wbytes = 2.0 * c.num_layers * (((double)Nqkv + Hl) * H + 3.0 * Fl * H) +
                            2.0 * V * H;
      wstream = wbytes > 192.0 * (1 << 20) ? FFMI_W_STREAM : 0;
      if (const char *e = getenv("FFMI_W_STREAM"))  // A/B override: 0 / 1
        wstream = atoi(e) ? FFMI_W_STREAM : 0;
    }
    TRY(ffmi_batch_create(Tm, o.max_requests, &chain_batch[0]));
    TRY(alloc(&res, (size_t)Tm * H));
    TRY(alloc(&h, (size_t)Tm * H));
    TRY(alloc(&qkv, (size_t)Tm * Nqkv));
    TRY(alloc(&att, (size_t)Tm * Hl));
    TRY(alloc(&proj, (size_t)Tm * H));
    TRY(alloc(&ss_o, (size_t)2 * 32 * (H / 16)));
    ss_d = ss_o + (size_t)32 * (H / 16);
    TRY(alloc(&mlp, (size_t)Tm * Fl));
    if (lora) {
      lora_tab_h.assign((size_t)c.num_layers * kLoraMods * FFMI_LORA_MAX_ADAPTERS, ffmi_lora_entry{});
      TRY(alloc(&lora_tab, lora_tab_h.size()));
      FFMI_HIP(hipMemset(lora_tab, 0, lora_tab_h.size() * sizeof(ffmi_lora_entry)));
      // (the largest site: down, o, or the three segments of qkv)
      TRY(alloc(&lora_ws, (std::max({ffmi::lora_workspace_bytes(Tm, Fl), ffmi::lora_workspace_bytes(Tm, Hl),
                                     3 * ffmi::lora_workspace_bytes(Tm, H)}) + 3) / 4));
    }
    // (a GQA handle does not fold the o projection in: the GEMM runs)
    fuse_ao = !native_gqa && P == 1 && d == 64 && H <= 1024 && H % 16 == 0 &&
              !(getenv("FFMI_FUSE_AO") && atoi(getenv("FFMI_FUSE_AO")) == 0);
    if (fuse_ao) {  // decode / beam steps (<= 64 rows); prefill blocks run the GEMM
      oslab_T = std::min(Tm, 64);
      TRY(alloc(&oslab, (size_t)heads_l * oslab_T * H));
    }
    Vl = P > 1 && V % P == 0 && (V / P) % 16 == 0 ? V / P : V;
    if (const char *e = getenv("FFMI_VOCAB_SHARD"))  // A/B: 0 = replicated lm_head
      if (!atoi(e)) Vl = V;
    TRY(alloc(&logits, (size_t)Tm * Vl));
    if (Vl != V) TRY(alloc(&xch, (ffmi_vocab_shard_scratch_bytes(P, Tm) + 3) / 4));
    TRY(alloc(&ids_d, (size_t)Tm * 4 * 2));  // [ids | probs] of a step, one D2H copy
    topk_ws_bytes = ffmi::argmax_workspace_bytes(std::min(Tm, 256));
    TRY(alloc((char **)&topk_ws, topk_ws_bytes));
    FFMI_HIP(hipMemsetAsync(topk_ws, 0, topk_ws_bytes, stream));
    peer = P > 1 && ffmi::comm_has_peer(o.comm, (size_t)Tm * H * 2);
    // an attached transport too small for this model's largest [Tm][H]
    // all-reduce needs RCCL (or the local group) for those steps: refuse at
    // creation rather than failing mid-serve
    if (P > 1 && !peer && ffmi::comm_peer_attached(o.comm) && !ffmi::comm_has_fallback(o.comm)) {
      ffmi_set_last_error("xGMI exchange buffer smaller than max_tokens x hidden fp16 and no "
                          "RCCL communicator", __FILE__, __LINE__);
      return FFMI_ERR_INVALID;
    }
    rccl = P > 1 && !peer && ffmi::comm_is_rccl(o.comm);
    // a shard over a one-rank communicator with no RCCL state (the per-rank
    // shard bench): every all-reduce is the identity, so o/down defer their
    // slabs to the residual norm exactly as at TP = 1
    solo = P > 1 && !peer && !rccl && ffmi::comm_size(o.comm) == 1;
    if (peer || rccl) {
      tp_chunks = 2;
      if (const char *e = getenv("FFMI_TP_OVERLAP")) tp_chunks = atoi(e) ? 2 : 1;
      if ((H / tp_chunks) % 32 != 0) tp_chunks = 1;
      FFMI_HIP(hipStreamCreateWithFlags(&comm_stream, hipStreamNonBlocking));
      ev_chunk.resize(tp_chunks);
      for (auto &e : ev_chunk) FFMI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      FFMI_HIP(hipEventCreateWithFlags(&ev_comm_done, hipEventDisableTiming));
      if (tp_chunks > 1) TRY(alloc(&chunk_buf, (size_t)Tm * H));
    }
    {
      // the split-K factor depends on the row-block count, so take the max
      // over every batch size the model can see
      for (int t = 16; t <= Tm; t += 16) {
        const size_t w1 = ffmi_linear_workspace_bytes(t, Nqkv, H, FFMI_EPI_NONE);
        const size_t w2 = ffmi_linear_workspace_bytes(t, H, Hl, FFMI_EPI_NONE);
        const size_t w3 = ffmi_linear_workspace_bytes(t, Fl, H, FFMI_EPI_SILU_MUL);
        const size_t w4 = ffmi_linear_workspace_bytes(t, H, Fl, FFMI_EPI_NONE);
        const size_t w5 = ffmi_linear_workspace_bytes(t, Vl, H, FFMI_EPI_NONE);
        ws_bytes = std::max(ws_bytes, std::max(std::max(std::max(w1, w2), std::max(w3, w4)), w5));
      }
      // the row-parallel column chunks over the xGMI transport defer their
      // split-K slabs to the all-reduce's copy-in on comm_stream while the
      // next chunk computes: one workspace region per chunk
      if (peer && ar_slabs && tp_chunks > 1) {
        const int Hc = H / tp_chunks;
        for (int t = 16; t <= Tm; t += 16)
          ws_chunk = std::max(ws_chunk, std::max(ffmi_linear_workspace_bytes(t, Hc, Hl, FFMI_EPI_NONE),
                                                 ffmi_linear_workspace_bytes(t, Hc, Fl, FFMI_EPI_NONE)));
        ws_chunk = (ws_chunk + 255) & ~(size_t)255;
        ws_bytes = std::max(ws_bytes, ws_chunk * tp_chunks);
      }
      if (ws_bytes) TRY(alloc(&ws, (ws_bytes + 3) / 4));
    }
    // coherent (uncached) pinned memory: the sampling kernel's stores go
    // straight over PCIe and are visible to the host once the stream has
    // synchronised, whatever HIP_HOST_COHERENT says
    FFMI_HIP(hipHostMalloc((void **)&ids_h, (size_t)kChain * Tm * 4 * 2 * sizeof(int32_t),
                           hipHostMallocCoherent | hipHostMallocMapped));
    if (mode == FFMI_MODEL_BEAM) TRY(alloc(&ids_dev, (size_t)kChain * Tm * 4));
    // the chained beam steps' staging batches, created here rather than on a
    // chain's first use: creating one clears its device blob on the legacy
    // stream, which fails -- and invalidates the capture -- while another
    // thread's model is capturing a graph (the TP shard threads of one
    // process, ffmi_comm_create_local, beside their SSMs)
    if (mode == FFMI_MODEL_BEAM && o.tp_size == 1)
      for (int i = 1; i < kChain; ++i)
        TRY(ffmi_batch_create(Tm, o.max_requests, &chain_batch[i]));
    // weights (seeded synthetic, orc_gen_weight spec), packed for MFMA
    uint16_t *tmp = nullptr;
    size_t tmp_elems = std::max((size_t)V * H, std::max((size_t)F * H, (size_t)H * H));
    TRY(alloc(&tmp, tmp_elems));
    // synthetic inits (ffmi_model_opts.weight_init; oracle orc_model_create_ex):
    // 1 scales o/down by 1/sqrt(2L); 2 (token chain) scales the embeddings by
    // 128, doubled while the layers' residual noise sqrt(L (H + 2F)) outgrows
    // LLaMA-7B's by the same factor (oracle.h orc_chain_embed_scale: the
    // chain's logit margin stays at least 7B's), and makes lm_head the
    // permuted unscaled embedding rows
    FFMI_CHECK(o.weight_init >= 0 && o.weight_init <= 2, FFMI_ERR_INVALID);
    const int kres = o.weight_init == 1 ? (FFMI_WKIND_DEPTH | c.num_layers) : 0;
    auto fill = [&](uint16_t *dst, size_t n, const std::string &name, int kind, int cols = 0,
                    uint64_t pa = 1, float scale = 1.0f) -> ffmi_status {
      if (!weights_folder.empty()) return load_tensor(dst, n, name);
      FFMI_CHECK(dst, FFMI_ERR_INVALID);
      FFMI_HIP(ffmi::launch_fill_weight(dst, n, ffmi::weight_key(name.c_str(), o.weight_seed), kind,
                                        stream, cols, pa, 17, scale));
      return FFMI_OK;
    };
    const bool chain = o.weight_init == 2 && weights_folder.empty();
    float chain_scale = 128.0f;
    for (long long f2 = 1; f2 * 32LL * (4096 + 2 * 11008) <
                           (long long)c.num_layers * (c.hidden + 2LL * c.intermediate);
         f2 *= 4)
      chain_scale *= 2.0f;
    TRY(alloc(&embed, (size_t)V * H));
    TRY(fill(embed, (size_t)V * H, "model.embed_tokens.weight", 0, 0, 1, chain ? chain_scale : 1.0f));
    TRY(alloc(&final_norm, H));
    TRY(fill(final_norm, H, "model.norm.weight", 1));
    TRY(alloc(&lm, ffmi_linear_packed_bytes(Vl, H) / 2));
    if (chain)
      TRY(fill(tmp, (size_t)V * H, "model.embed_tokens.weight", 0, H, 7919));
    else
      TRY(fill(tmp, (size_t)V * H, "lm_head.weight", 0));
    // vocab shard s: rows [s*Vl, (s+1)*Vl) (the whole table when replicated)
    FFMI_HIP(launch_pack_weight(tmp, H, Vl == V ? 0 : o.tp_rank * Vl, 0, Vl, H, lm, 1, 0,
                                (Vl + 15) / 16, stream));
    slots = 0;
    layers.resize(c.num_layers);
    const int s = o.tp_rank;
    for (int l = 0; l < c.num_layers; ++l) {
      Layer &L = layers[l];
      const std::string p = "model.layers." + std::to_string(l) + ".";
      TRY(alloc(&L.in_norm, H));
      TRY(fill(L.in_norm, H, p + "input_layernorm.weight", 1));
      TRY(alloc(&L.post_norm, H));
      TRY(fill(L.post_norm, H, p + "post_attention_layernorm.weight", 1));
      // qkv: [Q_s | K_s | V_s] rows of this shard (file_loader.cc:286-303)
      TRY(alloc(&L.wqkv, ffmi_linear_packed_bytes(Nqkv, H) / 2));
      const char *names[3] = {"self_attn.q_proj.weight", "self_attn.k_proj.weight",
                              "self_attn.v_proj.weight"};
      for (int q = 0; q < 3; ++q) {
        // (native GQA: the k/v tensors at their num_kv_heads * d rows, this
        // rank's K/V heads; otherwise H rows, replicated on load if GQA)
        const size_t rows = q > 0 && native_gqa ? (size_t)c.num_kv_heads * d : (size_t)H;
        const int Nl = q > 0 ? Hkv : Hl;  // this rank's rows of the tensor
        TRY(fill(tmp, rows * H, p + names[q], 0));
        // one allocation of Nqkv / 16 tiles per k-row: Q, K, V tiles side by side
        FFMI_HIP(launch_pack_weight(tmp, H, s * Nl, 0, Nl, H, L.wqkv, 1,
                                    (q > 0 ? Hl + (q - 1) * Hkv : 0) / 16, Nqkv / 16, stream));
      }
      // o_proj: row-parallel -> columns [s*Hl, (s+1)*Hl)
      TRY(alloc(&L.wo, ffmi_linear_packed_bytes(H, Hl) / 2));
      TRY(fill(tmp, (size_t)H * H, p + "self_attn.o_proj.weight", kres));
      FFMI_HIP(launch_pack_weight(tmp, H, 0, s * Hl, H, Hl, L.wo, 1, 0, H / 16, stream));
      // gate | up: column-parallel, interleaved 16-column tiles
      TRY(alloc(&L.wgu, 2 * ffmi_linear_packed_bytes(Fl, H) / 2));
      TRY(fill(tmp, (size_t)F * H, p + "mlp.gate_proj.weight", 0));
      FFMI_HIP(launch_pack_weight(tmp, H, s * Fl, 0, Fl, H, L.wgu, 2, 0, 2 * ((Fl + 15) / 16),
                                  stream));
      TRY(fill(tmp, (size_t)F * H, p + "mlp.up_proj.weight", 0));
      FFMI_HIP(launch_pack_weight(tmp, H, s * Fl, 0, Fl, H, L.wgu, 2, 1, 2 * ((Fl + 15) / 16),
                                  stream));
      // down: row-parallel -> columns [s*Fl, (s+1)*Fl) of [H][F]
      TRY(alloc(&L.wd, ffmi_linear_packed_bytes(H, Fl) / 2));
      TRY(fill(tmp, (size_t)H * F, p + "mlp.down_proj.weight", kres));
      FFMI_HIP(launch_pack_weight(tmp, F, 0, s * Fl, H, Fl, L.wd, 1, 0, H / 16, stream));
      ffmi_attn_cfg ac{};  // (zeroed: fields added to the ABI later default to 0)
      ac.mode = mode == FFMI_MODEL_TREE ? FFMI_ATTN_TREE
                                        : (mode == FFMI_MODEL_BEAM ? FFMI_ATTN_SPEC : FFMI_ATTN_INC);
      ac.num_heads = heads_l;
      ac.head_dim = d;
      ac.max_requests = o.max_requests;
      ac.max_seq_len = o.max_seq_len;
      ac.max_tree_tokens = mode == FFMI_MODEL_INC ? 0 : o.max_tree_tokens;
      ac.max_tokens = Tm;
      ac.qk_scale = 1.0f / sqrtf((float)d);
      ac.rope_theta = c.rope_theta;
      ac.rope_llama3 = c.rope_llama3;
      ac.rope_factor = c.rope_factor;
      ac.rope_low_freq_factor = c.rope_low_freq_factor;
      ac.rope_high_freq_factor = c.rope_high_freq_factor;
      ac.rope_original_max_pos = c.rope_original_max_pos;
      ac.out_layout = packed ? 1 : 0;
      TRY(ffmi_attn_create_gqa(&ac, kvh_l, &L.attn));  // (kvh_l == heads_l: ffmi_attn_create)
      int sl = 0;
      ffmi_attn_kv_ptrs(L.attn, nullptr, nullptr, &sl);
      slots = sl;
    }
    FFMI_HIP(hipStreamSynchronize(stream));
    // the staging buffer is not needed after init
    for (auto it = allocs.begin(); it != allocs.end(); ++it)
      if (*it == tmp) {
        (void)hipFree(tmp);
        allocs.erase(it);
        break;
      }
    return FFMI_OK;
  }

  // Chunk ch of a row-parallel GEMM computed in tp_chunks column chunks: its
  // GEMM on `stream` into *cb (a chunk = Hc / 16 consecutive tiles of the
  // H / 16 per k-row), then comm_stream waits for it, so the caller's
  // collective on comm_stream runs while the next chunk computes.  Over the
  // transport the chunk's split-K slabs (its own workspace region) are left in
  // *part for the collective's copy-in, with no reduce pass on this stream.
  // (FFMI_FAULT_TP_AR_DROP: the chunk zeroed before it is handed over)
  ffmi_status rowpar_chunk(const uint16_t *X, const uint16_t *W, int K, int T, int XP, int ch,
                           uint16_t **cb, ffmi::Partials *part) {
    const int H = c.hidden, Hc = H / tp_chunks;
    const size_t tiles = (size_t)(Hc / 16) * ffmi::w_tile_stride((K + 31) / 32);
    const bool drop = ar_drop_now;
    // (the norm variant runs over the transport only: peer is implied there)
    const bool def = peer && ar_slabs && !drop;
    *cb = chunk_buf + (size_t)ch * T * Hc;
    FFMI_HIP(ffmi::launch_gemm(X, W + ch * tiles, *cb,
                               def ? (float *)((char *)ws + ch * ws_chunk) : ws,
                               def ? ws_chunk : ws_bytes, T, Hc, K, XP, stream,
                               def ? part : nullptr, H / 16));
    if (drop) FFMI_HIP(hipMemsetAsync(*cb, 0, (size_t)T * Hc * 2, stream));
    FFMI_HIP(hipEventRecord(ev_chunk[ch], stream));
    FFMI_HIP(hipStreamWaitEvent(comm_stream, ev_chunk[ch], 0));
    return FFMI_OK;
  }
  // `stream` behind the chunks' collectives
  ffmi_status rowpar_join() {
    FFMI_HIP(hipEventRecord(ev_comm_done, comm_stream));
    FFMI_HIP(hipStreamWaitEvent(stream, ev_comm_done, 0));
    return FFMI_OK;
  }

  // Row-parallel GEMM + sum all-reduce into `out` [T][H] (model.cc:3421-3445).
  // Over the xGMI transport the output columns are computed in tp_chunks
  // halves: half c goes to comm_stream for its all-reduce (strided into
  // `out`) as soon as its GEMM is done, while half c + 1 computes.
  ffmi_status rowpar_gemm_allreduce(const uint16_t *X, const uint16_t *W, int K, uint16_t *out,
                                    int T, int XP) {
    const int H = c.hidden;
    if (!(peer || rccl) || tp_chunks == 1) {
      // (FFMI_FAULT_TP_AR_DROP: the GEMM's output zeroed before the all-reduce)
      const bool drop = ar_drop_now;
      // over the transport the split-K reduce is the all-reduce's copy-in
      ffmi::Partials part;
      FFMI_HIP(ffmi::launch_gemm(X, W, out, ws, ws_bytes, T, H, K, XP, stream,
                                 peer && ar_slabs && !drop ? &part : nullptr));
      if (drop) FFMI_HIP(hipMemsetAsync(out, 0, (size_t)T * H * 2, stream));
      if (peer)
        return ffmi::comm_allreduce_cols(o.comm, out, out, T, H, H, 0, FFMI_F16, stream,
                                         part.S > 0 ? &part : nullptr);
      return ffmi_allreduce(o.comm, out, out, (size_t)T * H, FFMI_F16, (ffmi_stream)stream);
    }
    const int Hc = H / tp_chunks;
    for (int ch = 0; ch < tp_chunks; ++ch) {
      uint16_t *cb;
      ffmi::Partials part;
      TRY(rowpar_chunk(X, W, K, T, XP, ch, &cb, &part));
      if (peer) {  // the transport reduces straight into out's columns
        TRY(ffmi::comm_allreduce_cols(o.comm, cb, out, T, Hc, H, ch * Hc, FFMI_F16, comm_stream,
                                      part.S > 0 ? &part : nullptr));
      } else {  // RCCL: contiguous in place, then into out's columns
        TRY(ffmi_allreduce(o.comm, cb, cb, (size_t)T * Hc, FFMI_F16, (ffmi_stream)comm_stream));
        FFMI_HIP(hipMemcpy2DAsync(out + (size_t)ch * Hc, (size_t)H * 2, cb, (size_t)Hc * 2,
                                  (size_t)Hc * 2, T, hipMemcpyDeviceToDevice, comm_stream));
      }
    }
    return rowpar_join();
  }

  // rowpar_gemm_allreduce with the residual norm after it folded into the
  // transport's all-reduce (tp_fuse_norm): res += sum (this rank's rows in
  // two-shot mode), h = RMSNorm(res) * wnorm on every rank.  Column chunks:
  // chunk 0 is reduced on comm_stream (two-shot: only this rank's rows) while
  // chunk 1 computes; chunk 1's all-reduce carries the norm, reading chunk 0's
  // columns of the sum from proj.
  ffmi_status rowpar_gemm_allreduce_norm(const uint16_t *X, const uint16_t *W, int K, int T, int XP,
                                         const uint16_t *wnorm) {
    const int H = c.hidden;
    const float eps = c.rms_eps;
    const bool two = ffmi::comm_two_shot(o.comm, (size_t)T * H * 2);
    if (tp_chunks == 1) {
      const bool drop = ar_drop_now;
      ffmi::Partials part;
      FFMI_HIP(ffmi::launch_gemm(X, W, proj, ws, ws_bytes, T, H, K, XP, stream,
                                 ar_slabs && !drop ? &part : nullptr));
      if (drop) FFMI_HIP(hipMemsetAsync(proj, 0, (size_t)T * H * 2, stream));
      return ffmi::comm_allreduce_norm(o.comm, proj, T, H, 0, nullptr, res, wnorm, eps, h, packed,
                                       two, stream, part.S > 0 ? &part : nullptr);
    }
    const int Hc = H / tp_chunks;
    const int nr = ffmi::comm_size(o.comm), rk = ffmi::comm_rank(o.comm);
    for (int ch = 0; ch < tp_chunks; ++ch) {
      uint16_t *cb;
      ffmi::Partials part;
      TRY(rowpar_chunk(X, W, K, T, XP, ch, &cb, &part));
      const ffmi::Partials *sl = part.S > 0 ? &part : nullptr;
      if (ch + 1 < tp_chunks)  // columns [ch Hc, (ch+1) Hc) of the sum into proj
        TRY(two ? ffmi::comm_reduce_rows(o.comm, cb, proj, T, Hc, H, ch * Hc,
                                         (int)((long)T * rk / nr), (int)((long)T * (rk + 1) / nr),
                                         comm_stream, sl)
                : ffmi::comm_allreduce_cols(o.comm, cb, proj, T, Hc, H, ch * Hc, FFMI_F16,
                                            comm_stream, sl));
      else
        TRY(ffmi::comm_allreduce_norm(o.comm, cb, T, H, ch * Hc, proj, res, wnorm, eps, h, packed,
                                      two, comm_stream, sl));
    }
    return rowpar_join();
  }

  // One step over the packed batch; k = results per token.  Small batches
  // (SSM beam steps, decode) are launch-bound -- ~20 kernels of a few us
  // each -- so their whole step (metadata copy, kernels, result copies) is
  // captured once per batch shape into a HIP graph and replayed.
  struct GraphKey {
    int T, W, C, k, parity, overlap, fused, max_q, slot;
    size_t bytes;
    int lora_mask = 0;  // (FFMI_MODEL_LORA: the modules whose route the step takes, lora_route)
    bool operator<(const GraphKey &o) const {
      return std::tie(T, W, C, k, parity, overlap, fused, max_q, slot, bytes, lora_mask) <
             std::tie(o.T, o.W, o.C, o.k, o.parity, o.overlap, o.fused, o.max_q, o.slot, o.bytes,
                      o.lora_mask);
    }
  };
  // TREE steps write alternate halves of the attention staging (commits of
  // the next step read the half this one wrote); kept here so graph replays
  // and eager steps agree
  int tree_parity = 0;
  GraphCache<GraphKey> graphs{512};
  // FFMI_CHAIN_GROUP=g (>= 2): chained beam slots 1 .. kChain-2 are staged and
  // go out g per graph launch (slot kChain-1 alone, behind the collect event):
  // the boundary between two graph launches (4.9 us from one step's last
  // kernel to the next step's first, profiles/r06_ssm_gaps.log) becomes a
  // kernel boundary inside one graph.  1 = one launch per slot.  Default: all
  // six middle slots in one launch (the host stages them while slot 0 runs).
  // Same box, 3 pairs (profiles/r06_chain_group_ab.log): SSM step 95.8-97.8
  // (1 per launch) -> 93.8-94.5 (3) -> 92.9-93.9 us (6); 1325-1330 -> 1332-1336
  // tokens/s
  int chain_group = getenv("FFMI_CHAIN_GROUP") ? atoi(getenv("FFMI_CHAIN_GROUP")) : kChain - 2;
  struct PendingSlot {
    Step step;
    GraphKey key;
  };
  std::vector<PendingSlot> pend;  // staged, not yet launched (grouped slots)
  GraphCache<std::vector<GraphKey>> group_graphs{256};
  bool use_graphs = getenv("FFMI_NO_GRAPHS") == nullptr;
  bool blob_fetch = !getenv("FFMI_BLOB_FETCH") || atoi(getenv("FFMI_BLOB_FETCH")) != 0;
  // largest one-item-per-request step that is graphed (FFMI_GRAPH_MAXT: A/B)
  int graph_max_t = getenv("FFMI_GRAPH_MAXT") ? atoi(getenv("FFMI_GRAPH_MAXT")) : 1024;

  // forward = forward_launch (stage the step, enqueue it) + forward_finish
  // (wait for it); SSM beam steps of several SSMs launch all, then finish
  // each (serve_spec_infer), so their latency-bound steps overlap
  bool inflight = false;
  // FFMI_STEP_TIMING=1 (diagnostics): per step, host time spent staging and
  // launching, the GPU span between events around the launch, and the
  // host's wait; summed per step size and printed at destruction
  bool step_timing = getenv("FFMI_STEP_TIMING") && atoi(getenv("FFMI_STEP_TIMING")) != 0;
  hipEvent_t st_ev[2] = {nullptr, nullptr};
  double st_t0 = 0, st_t1 = 0;
  struct StepTime { long n = 0; double launch = 0, gpu = 0, wait = 0, total = 0; };
  std::map<int, StepTime> st_sum;
  int st_T = 0;
  ffmi_status forward(int k) {
    TRY(forward_launch(k, 0));
    return forward_finish();
  }

  // a side array behind what is staged in b so far (16-byte aligned pieces)
  template <typename E>
  static ffmi_status stage_extra(StepExtra<E> *x, int T, ffmi_batch_dev *b, size_t *bytes) {
    x->off = *bytes;
    const size_t n = ((size_t)T * sizeof(E) + 15) & ~(size_t)15;
    FFMI_CHECK((int)x->v.size() == T && *bytes + n <= b->cap, FFMI_ERR_INVALID);
    memcpy(b->host + *bytes, x->v.data(), (size_t)T * sizeof(E));
    *bytes += n;
    return FFMI_OK;
  }

  // Stage the packed batch (ps) as the step of `slot`, k results per token:
  // the records, then the side arrays that are switched on -- draws, targets,
  // adapter ids, in that order.  A BEAM step never has any: set_sampling and
  // set_logprobs refuse a BEAM model and creation refuses FFMI_MODEL_LORA on
  // one, so a chained or grouped slot's blob is its records alone and its key
  // has lora_mask = 0.  *key is set for a step with rows only.
  ffmi_status stage_step(int k, int slot, Step *s, GraphKey *key) {
    const int T = (int)ps.tokens.size();
    ffmi_batch_dev *b = chain_batch[slot];
    ffmi_batch_desc desc;
    ps.desc(&desc);
    // the embedding gather indexes the table by token id: reject bad ids on
    // the host instead of reading out of bounds on the device
    // (a chained beam step's -1 - i: entry i of the previous slot's ids,
    // themselves top-k picks in range)
    const long prev_n = slot > 0 ? (long)slot_results[slot - 1] : 0;
    for (int t = 0; t < T; ++t)
      FFMI_CHECK((desc.tokens[t].token_id >= 0 && desc.tokens[t].token_id < c.vocab_size) ||
                     (desc.tokens[t].token_id < 0 && -1L - desc.tokens[t].token_id < prev_n),
                 FFMI_ERR_INVALID);
    size_t bytes = 0;
    TRY(ffmi::batch_stage(b, &desc, &bytes));
    *s = Step{b, slot, T, k, bytes};
    if (T == 0) return FFMI_OK;
    if (sampling) TRY(stage_extra(&step_u, T, b, &bytes));
    if (logprobs) TRY(stage_extra(&step_targets, T, b, &bytes));
    if (lora) TRY(stage_extra(&step_slots, T, b, &bytes));
    s->blob_bytes = bytes;
    *key = GraphKey{T, b->num_work, b->num_commits, k, tree_parity, b->commit_overlap ? 1 : 0,
                    (b->one_item_per_req ? 1 : 0) | (b->lds_tail ? 2 : 0), b->max_q, slot, bytes,
                    (int)lora_route()};
    return FFMI_OK;
  }

  ffmi_status forward_launch(int k, int slot) {
    inflight = false;
    const int T = (int)ps.tokens.size();
    if (step_timing) {
      if (!st_ev[0]) {
        FFMI_HIP(hipEventCreate(&st_ev[0]));
        FFMI_HIP(hipEventCreate(&st_ev[1]));
      }
      st_t0 = now_us();
      st_T = T;
    }
    prof_this_step = prof_level == 1 && (prof_steps++ % prof_every) == 0;
    Step step;
    GraphKey key{};
    TRY(stage_step(k, slot, &step, &key));
    if (T == 0) return FFMI_OK;
    // graphed: small steps, and tree-verify steps of one work item per
    // request (a fixed shape while the batch is full: T = 168 for 8 requests
    // of 21 tree tokens); prefill blocks stay eager (one-off shapes)
    const bool graph = use_graphs && !dbg &&
                       (T <= 64 || (step.batch->one_item_per_req && T <= graph_max_t)) &&
                       (o.tp_size == 1 || peer || rccl || ffmi::comm_size(o.comm) == 1) &&
                       !prof_on(0, T) &&
                       !prof_on(c.num_layers / 2, T);
    hipGraphExec_t ex = nullptr;
    if (graph && !(ex = graphs.find(key))) {
      if (graphs.full()) clear_graphs();
      TRY(capture_graph(stream, [&] { return enqueue(step, false); }, &ex));
      graphs.insert(key, ex);
    }
    if (step_timing) FFMI_HIP(hipEventRecord(st_ev[0], stream));
    if (graph) FFMI_HIP(hipGraphLaunch(ex, stream));
    else TRY(enqueue(step, true));
    if (step_timing) {
      FFMI_HIP(hipEventRecord(st_ev[1], stream));
      st_t1 = now_us();
    }
    inflight = true;
    return FFMI_OK;
  }

  // A chained slot staged for a grouped launch (chain_group); flush_pending
  // captures / replays the group.
  ffmi_status stage_pending(int k, int slot) {
    PendingSlot q{};
    const ffmi_status st = stage_step(k, slot, &q.step, &q.key);
    if (st == FFMI_OK) pend.push_back(q);
    return st;
  }
  ffmi_status flush_pending() {
    if (pend.empty()) return FFMI_OK;
    std::vector<GraphKey> keys;
    for (const auto &q : pend) keys.push_back(q.key);
    hipGraphExec_t ex = group_graphs.find(keys);
    if (!ex) {
      if (group_graphs.full()) clear_graphs();
      const ffmi_status st = capture_graph(stream, [&]() -> ffmi_status {
        for (const auto &q : pend) {
          const ffmi_status e = enqueue(q.step, false);
          if (e != FFMI_OK) return e;
        }
        return FFMI_OK;
      }, &ex);
      if (st != FFMI_OK) {
        pend.clear();
        return st;
      }
      group_graphs.insert(keys, ex);
    }
    pend.clear();
    FFMI_HIP(hipGraphLaunch(ex, stream));
    inflight = true;
    return FFMI_OK;
  }

  ffmi_status forward_finish() {
    if (!inflight) return FFMI_OK;
    inflight = false;
    ffmi_status st;
    const double tw = step_timing ? now_us() : 0;
    FFMI_HIP(hipStreamSynchronize(stream));
    if (step_timing) {
      const double te = now_us();
      float ms = 0;
      (void)hipEventElapsedTime(&ms, st_ev[0], st_ev[1]);
      StepTime &q = st_sum[st_T];
      q.n++;
      q.launch += st_t1 - st_t0;
      q.gpu += ms * 1e3;
      q.wait += te - tw;
      q.total += te - st_t0;
    }
    // any attached transport (also under the RCCL path, whose chunks that fit
    // the exchange buffer still go over it) reports timeouts / errors here
    if ((peer || (o.comm && ffmi::comm_peer_attached(o.comm))) &&
        (st = ffmi::comm_status(o.comm)) != FFMI_OK)
      return st;
    if (mode == FFMI_MODEL_TREE) tree_parity ^= 1;
    if (!recs.empty()) prof_collect();
    return FFMI_OK;
  }

  void clear_graphs() {
    graphs.clear();
    group_graphs.clear();
  }

  // everything a step puts on the stream (no host synchronisation inside)
  ffmi_status enqueue(const Step &step, bool record_upload) {
    const int H = c.hidden, V = c.vocab_size, T = step.T;
    ffmi_batch_dev *const batch = step.batch;
    const size_t blob_bytes = step.blob_bytes;
    const float eps = c.rms_eps;
    const ffmi_stream s = (ffmi_stream)stream;
    // the step's blob: fetched by the first kernel from the mapped staging
    // (default), or a separate H2D copy (FFMI_BLOB_FETCH=0: A/B)
    if (!blob_fetch) TRY(ffmi::batch_copy(batch, blob_bytes, stream, record_upload));
    const bool ptail = prof_on(0, T);
    int pr = 0;
    ffmi::Partials down_part;
    // FFMI_MARKERS=<hidden>: clock markers between the last layer's kernels
    // of the model with that hidden size (diagnostics, ffmi_debug_markers)
    // (FFMI_MARKERS_T: only steps of that many tokens, e.g. 168 = a full
    // verify batch; the attention stamps then come from the same launch)
    static const int marker_h = getenv("FFMI_MARKERS") ? atoi(getenv("FFMI_MARKERS")) : 0;
    static const int marker_t = getenv("FFMI_MARKERS_T") ? atoi(getenv("FFMI_MARKERS_T")) : 0;
    int mark_i = 0;
    const bool fuse = (fuse_norms == 2 || (fuse_norms == 1 && H >= 2048)) && !dbg &&
                      o.tp_size == 1 && T <= 32 && H % 32 == 0 && Hl % 32 == 0 && H <= 4096;
    // (FFMI_MODEL_LORA, the modules of the step's route, lora_route.  down: it
    // runs unfused and its split-K slabs are reduced into proj for the update,
    // so the norm after it -- the next layer's attention norm, the final norm
    // -- is a launch again.  o: the same for the o projection and the
    // post-attention norm, and gate/up then reads the norm's output; an o
    // projection folded into the attention stays there, its per-head slabs
    // reduced into proj.  q / k / v: the attention norm is a launch, the qkv
    // GEMM writes reduced fp16 rows and the update runs on them before the
    // attention.  A step with an empty route is the step of a model without
    // the flag)
    const unsigned lroute = lora_route();
    const bool lora_step = (lroute & FFMI_LORA_DOWN_BIT) != 0, lora_o = (lroute & FFMI_LORA_O_BIT) != 0,
               lora_qkv = (lroute & kLoraQKV) != 0;
    const bool fuse_d = fuse && !lora_step, fuse_o = fuse && !lora_o;
    const int32_t *const lslots =
        lora ? reinterpret_cast<const int32_t *>(step.batch->dev + step_slots.off) : nullptr;
    // the residual norms inside the transport's all-reduces (tp_fuse_norm)
    const bool arn = peer && !solo && o.tp_size > 1 && (tp_fuse_norm == 2 || (tp_fuse_norm == 1 && !dbg));
    for (int l = 0; l < c.num_layers; ++l) {
      Layer &L = layers[l];
      const bool on = prof_on(l, T);
      const bool mark_on = marker_h == c.hidden && l == c.num_layers - 1 && (!marker_t || T == marker_t);
      if (marker_h) ffmi::attn_stamp_gate(mark_on);
      auto mk = [&]() {
        if (mark_on) (void)ffmi::launch_marker(mark_i++, stream);
      };
      // (the marker buffer is allocated by an eager launch, never in a capture)
      if (marker_h && l == 0 && record_upload) (void)ffmi::launch_marker(63, stream);
      mk();
      // split-K GEMMs leave their partial slabs for the next kernel to combine
      // (rope-store for qkv; the residual norm for o/down when there is no
      // all-reduce in between) instead of a separate reduce pass
      const int XP = (packed ? FFMI_X_PACKED : 0) | wstream;
      // fused residual norms (see fuse_norms): from layer 1 on, the attention
      // norm is the qkv GEMM's prologue on the residual the down projection
      // left, and every post-attention norm the gate/up GEMM's
      const bool fz_in = fuse_d && l > 0 && !lora_qkv;
      ffmi::FuseArgs fz_qkv, fz_o, fz_gu, fz_d;
      if (fuse) {
        fz_o.kind = fz_d.kind = 1;
        fz_o.res_in = fz_d.res_in = res;
        fz_o.ss_out = ss_o, fz_d.ss_out = ss_d;
        fz_qkv.kind = fz_gu.kind = 2;
        fz_qkv.ss_in = ss_d, fz_gu.ss_in = ss_o;
        fz_qkv.nss = fz_gu.nss = H / 16;
        fz_qkv.wnorm = L.in_norm, fz_gu.wnorm = L.post_norm;
        fz_qkv.eps = fz_gu.eps = eps;
      }
      if (fuse_d && l > 0 && lora_qkv) {  // (res holds the residual add: the norm alone)
        pr = prof_begin(on);
        FFMI_HIP(ffmi::launch_rmsnorm(res, nullptr, L.in_norm, nullptr, h, T, H, eps, stream, packed));
        prof_end(pr, NORM, (double)T * H * 2 * 2, 0);
        mk();
      } else if (!fz_in && !(arn && l > 0)) {  // (arn: the previous down all-reduce normalised)
        pr = prof_begin(on);
        // layer 0: the embedding lookup gathers straight into the first norm
        // (embedding_kernels.cu:233-244; res = the looked-up rows)
        FFMI_HIP(ffmi::launch_rmsnorm(l == 0 ? embed : res, l == 0 ? nullptr : proj, L.in_norm, res,
                                      h, T, H, eps, stream, packed,
                                      l == 0 ? ffmi::Partials() : down_part,
                                      l == 0 ? (blob_fetch ? batch->host : batch->dev) : nullptr,
                                      l == 0 && blob_fetch ? batch->dev : nullptr, blob_bytes,
                                      step.slot > 0 ? slot_ids_dev(step.slot - 1) : nullptr));
        // the staging is free for the next step once the fetch has read it
        if (l == 0 && blob_fetch && record_upload) FFMI_HIP(hipEventRecord(batch->uploaded, stream));
        prof_end(pr, NORM, (double)T * H * 2 * (l == 0 ? 3 : 4), 0);
        mk();
      }
      if (dbg) {
        // residual stream after layer l-1 (layer 0: the embedding rows; arn:
        // current on this rank's rows only, not kept)
        if (l == 0 || !arn) TRY(dbg_copy(l == 0 ? FFMI_DBG_EMBED : FFMI_DBG_HIDDEN, l == 0 ? 0 : l - 1, res, T));
        TRY(dbg_copy(FFMI_DBG_ATTN_NORM, l, h, T));
      }
      pr = prof_begin(on);
      ffmi::Partials qkv_part;
      // (a GQA handle takes fp16 qkv rows: a split-K plan runs its reduce pass)
      FFMI_HIP(ffmi::launch_gemm(fz_in ? res : h, L.wqkv, qkv, (float *)ws, ws_bytes, T, Nqkv, H,
                                 fz_in ? wstream : XP, stream,
                                 native_gqa || lora_qkv ? nullptr : &qkv_part, 0,
                                 fz_in ? &fz_qkv : nullptr));
      prof_end(pr, GEMM_QKV, gemm_bytes(T, Nqkv, Nqkv, H), 2.0 * T * Nqkv * H);
      if (lora_qkv) {  // qkv += scale * (h A^T) B^T per segment, ahead of RoPE and the KV store
        pr = prof_begin(on);
        const int w[3] = {Hl, Hkv, Hkv};
        const ffmi_lora_entry *tabs[3];
        for (int g = 0; g < 3; ++g) tabs[g] = lora_tab + lora_tab_at(l, g, 0);
        FFMI_HIP(ffmi::launch_lora_qkv(h, T, H, w, Nqkv, lslots, tabs, qkv, packed, lora_ws, nullptr,
                                       stream));
        prof_end(pr, LORA, 2.0 * FFMI_LORA_MAX_RANK * (3.0 * H + Nqkv) + 4.0 * T * Nqkv, 0);
      }
      mk();
      if (dbg) TRY(dbg_gemm_out(FFMI_DBG_QKV, l, qkv, qkv_part, T));
      pr = prof_begin(on);
      ffmi::OprojArgs oa;
      if (fuse_ao && !fuse_o) {
        oa.wo = L.wo, oa.slab = oslab, oa.N = H, oa.max_T = oslab_T;
        oa.wts = ffmi::w_tile_stride(Hl / 32), oa.wks = ffmi::w_k_stride(H / 16);
      }
      TRY(ffmi::attn_forward(L.attn, batch, qkv, qkv_part, att, s,
                             mode == FFMI_MODEL_TREE ? tree_parity : -1,
                             oa.wo ? &oa : nullptr));
      prof_end(pr, ATTENTION, on ? attn_bytes() : 0, 0);
      mk();
      if (dbg) TRY(dbg_copy(FFMI_DBG_ATTN_OUT, l, att, T));
      ffmi::Partials o_part;
      if (oa.done) {  // the attention projected: one slab per head
        o_part.p = oslab, o_part.S = heads_l, o_part.NP = H;
      } else if (fuse_o) {  // o projection + residual add (+ sums of squares): res in place
        pr = prof_begin(on);
        FFMI_HIP(ffmi::launch_gemm(att, L.wo, res, (float *)ws, ws_bytes, T, H, Hl, XP, stream,
                                   nullptr, 0, &fz_o));
        prof_end(pr, GEMM_O, gemm_bytes(T, H, H, Hl), 2.0 * T * H * Hl);
        mk();
      } else if (o.tp_size == 1 || solo) {
        pr = prof_begin(on);
        FFMI_HIP(ffmi::launch_gemm(att, L.wo, proj, (float *)ws, ws_bytes, T, H, Hl, XP, stream,
                                   H <= 8192 ? &o_part : nullptr));
        prof_end(pr, GEMM_O, gemm_bytes(T, H, H, Hl), 2.0 * T * H * Hl);
        mk();
      } else {  // GEMM + all-reduce (overlapped over xGMI): timed together
        pr = prof_begin(on);
        ar_drop_now = l == ar_drop_layer && ar_drop_which == 0;
        if (arn) TRY(rowpar_gemm_allreduce_norm(att, L.wo, Hl, T, XP, L.post_norm));
        else TRY(rowpar_gemm_allreduce(att, L.wo, Hl, proj, T, XP));
        ar_drop_now = false;
        prof_end(pr, ALLREDUCE, gemm_bytes(T, H, H, Hl), 2.0 * T * H * Hl);
        mk();
      }
      if (lora_o) {  // proj += scale * (att A^T) B^T on the rows with an o adapter
        pr = prof_begin(on);
        // (split-K or per-head slabs summed in order and rounded once: the
        // fp16 value the residual norm computes from them)
        if (o_part.S > 0) {
          FFMI_HIP(ffmi::launch_partials_reduce(o_part, proj, T, H, stream));
          o_part = ffmi::Partials();
        }
        FFMI_HIP(ffmi::launch_lora(att, T, Hl, H, lslots, lora_tab + lora_tab_at(l, FFMI_LORA_O, 0),
                                   proj, packed, lora_ws, nullptr, stream));
        prof_end(pr, LORA, 2.0 * FFMI_LORA_MAX_RANK * ((double)Hl + H) + 4.0 * T * H, 0);
        mk();
      }
      if (dbg && !arn) TRY(dbg_gemm_out(FFMI_DBG_O_PROJ, l, proj, o_part, T));
      if (!fuse_o && !arn) {
        pr = prof_begin(on);
        FFMI_HIP(ffmi::launch_rmsnorm(res, proj, L.post_norm, res, h, T, H, eps, stream, packed,
                                      o_part));
        prof_end(pr, NORM, (double)T * H * 2 * 4, 0);
        mk();
      }
      if (dbg) TRY(dbg_copy(FFMI_DBG_FFN_NORM, l, h, T));
      pr = prof_begin(on);
      const int YP = packed ? FFMI_Y_PACKED : 0;
      if (fuse_o)
        FFMI_HIP(ffmi::launch_gemm(res, L.wgu, mlp, (float *)ws, ws_bytes, T, Fl, H,
                                   FFMI_EPI_SILU_MUL | YP | wstream, stream, nullptr, 0, &fz_gu));
      else
        TRY(ffmi_linear_ws(h, L.wgu, mlp, T, Fl, H, FFMI_EPI_SILU_MUL | XP | YP, ws, ws_bytes, s));
      prof_end(pr, GEMM_GATE_UP, gemm_bytes(T, 2 * Fl, Fl, H), 2.0 * T * 2 * Fl * H);
      mk();
      if (dbg) TRY(dbg_copy(FFMI_DBG_MLP_ACT, l, mlp, T));
      if (fuse_d) {  // down projection + residual add (+ sums of squares)
        pr = prof_begin(on);
        FFMI_HIP(ffmi::launch_gemm(mlp, L.wd, res, (float *)ws, ws_bytes, T, H, Fl, XP, stream,
                                   nullptr, 0, &fz_d));
        prof_end(pr, GEMM_DOWN, gemm_bytes(T, H, H, Fl), 2.0 * T * H * Fl);
        mk();
        mk();
      } else if (o.tp_size == 1 || solo) {
        pr = prof_begin(on);
        FFMI_HIP(ffmi::launch_gemm(mlp, L.wd, proj, (float *)ws, ws_bytes, T, H, Fl, XP, stream,
                                   H <= 8192 ? &down_part : nullptr));
        prof_end(pr, GEMM_DOWN, gemm_bytes(T, H, H, Fl), 2.0 * T * H * Fl);
        if (lora_step) {  // proj += scale * (mlp A^T) B^T on the rows with an adapter
          pr = prof_begin(on);
          // (the slabs summed in slab order and rounded once: the fp16 value
          // every consumer of the slabs computes, so rows without an adapter
          // keep the bits of a step without adapters)
          if (down_part.S > 0) {
            FFMI_HIP(ffmi::launch_partials_reduce(down_part, proj, T, H, stream));
            down_part = ffmi::Partials();
          }
          FFMI_HIP(ffmi::launch_lora(mlp, T, Fl, H, lslots,
                                     lora_tab + lora_tab_at(l, FFMI_LORA_DOWN, 0), proj, packed,
                                     lora_ws, nullptr, stream));
          prof_end(pr, LORA, 2.0 * FFMI_LORA_MAX_RANK * ((double)Fl + H) + 4.0 * T * H, 0);
        }
        mk();
        mk();  // (two back to back: the marker-to-marker boundary itself)
      } else {
        pr = prof_begin(on);
        ar_drop_now = l == ar_drop_layer && ar_drop_which == 1;
        // (arn: the next layer's input norm, or the final norm, rides along)
        if (arn)
          TRY(rowpar_gemm_allreduce_norm(mlp, L.wd, Fl, T, XP,
                                         l + 1 < c.num_layers ? layers[l + 1].in_norm : final_norm));
        else TRY(rowpar_gemm_allreduce(mlp, L.wd, Fl, proj, T, XP));
        ar_drop_now = false;
        prof_end(pr, ALLREDUCE, gemm_bytes(T, H, H, Fl), 2.0 * T * H * Fl);
        mk();
      }
      if (dbg && !arn) TRY(dbg_gemm_out(FFMI_DBG_DOWN, l, proj, down_part, T));
    }
    const int XP = (packed ? FFMI_X_PACKED : 0) | wstream;
    // (markers also between the tail's kernels: final norm, lm_head, sampling)
    const bool tail_mark = marker_h == c.hidden && (!marker_t || T == marker_t);
    auto mkt = [&]() {
      if (tail_mark) (void)ffmi::launch_marker(mark_i++, stream);
    };
    if (!arn) {  // (arn: the last down all-reduce applied the final norm)
      pr = prof_begin(ptail);
      if (fuse_d)  // res already holds the last residual add
        FFMI_HIP(ffmi::launch_rmsnorm(res, nullptr, final_norm, nullptr, h, T, H, eps, stream, packed));
      else
        FFMI_HIP(ffmi::launch_rmsnorm(res, proj, final_norm, res, h, T, H, eps, stream, packed,
                                      down_part));
      prof_end(pr, NORM, (double)T * H * 2 * 4, 0);
    }
    mkt();
    if (dbg) {
      if (!arn) TRY(dbg_copy(FFMI_DBG_HIDDEN, c.num_layers - 1, res, T));
      TRY(dbg_copy(FFMI_DBG_HIDDEN, c.num_layers, h, T));
      dbg_T = T;
    }
    pr = prof_begin(ptail);
    TRY(ffmi_linear_ws(h, lm, logits, T, Vl, H, FFMI_EPI_NONE | XP, ws, ws_bytes, s));
    prof_end(pr, GEMM_LM_HEAD, gemm_bytes(T, Vl, Vl, H), 2.0 * T * Vl * H);
    mkt();
    pr = prof_begin(ptail);
    TRY(enqueue_sampling(step));
    prof_end(pr, SAMPLING, (double)T * V * 2, 0);
    mkt();
    if (logprobs) {
      pr = prof_begin(ptail);
      TRY(enqueue_logprobs(step));
      prof_end(pr, LOGPROBS, (double)T * V * 2, 0);
    }
    return FFMI_OK;
  }

  // softmax + argmax / arg-top-k of the step's logits into the pinned results
  ffmi_status enqueue_sampling(const Step &step) {
    const int V = c.vocab_size, T = step.T, k = step.k;
    const ffmi_batch_dev *batch = step.batch;
    const ffmi_stream s = (ffmi_stream)stream;
    // ids [T*k] then probs [T*k] back to back.  The sampling kernel writes
    // them straight into the pinned host buffer (a few bytes per row over
    // PCIe, visible after the stream synchronisation like a copy kernel's
    // stores), so a step needs no result-copy launch; FFMI_RESULT_COPY=1
    // keeps the device buffer + copy (A/B runs)
    int32_t *ids_o = result_copy ? ids_d : slot_ids_h(step.slot);
    float *probs_o = reinterpret_cast<float *>(ids_o + (size_t)T * k);
    if (sampling && Vl != V) {
      // sharded top-p: five record exchanges; every rank staged the same u
      FFMI_CHECK(k == 1 && sample_ws, FFMI_ERR_INVALID);
      TRY(ffmi_vocab_shard_sample_topp(
          o.comm, logits, T, Vl, temperature, topp,
          reinterpret_cast<const float *>(batch->dev + step_u.off), ids_o, probs_o, sample_ws,
          sample_ws_bytes, s));
    } else if (sampling) {
      // (set_sampling: INC; u behind the blob's records)
      FFMI_CHECK(k == 1 && sample_ws, FFMI_ERR_INVALID);
      FFMI_HIP(ffmi::launch_sample_topp(
          logits, T, V, temperature, topp, reinterpret_cast<const float *>(batch->dev + step_u.off),
          ids_o, probs_o, sample_ws, ffmi::sample_topp_workspace_bytes(T, V), stream));
    } else if (Vl != V) {
      // sharded softmax / top-k: three record exchanges, then the merge
      TRY(ffmi_vocab_shard_topk(o.comm, logits, T, Vl, k, ids_o, probs_o, xch, s));
    } else {
      // the ids also to device memory: the next chained beam step's
      // embedding gather reads them there
      FFMI_CHECK(k >= 1 && k <= 4 && k <= V, FFMI_ERR_INVALID);
      FFMI_HIP(ffmi::launch_argmax(logits, T, V, k, ids_o, probs_o, stream, topk_ws, topk_ws_bytes,
                                   mode == FFMI_MODEL_BEAM
                                       ? slot_ids_dev(step.slot)
                                       : logprobs ? lp_picks : nullptr));
    }
    if (result_copy)
      FFMI_HIP(hipMemcpyAsync(slot_ids_h(step.slot), ids_d, (size_t)T * k * 8,
                              hipMemcpyDeviceToHost, stream));
    return FFMI_OK;
  }

  // the log-probability of every row's scored id, behind the pick
  // (set_logprobs: INC / TREE, Vl == V, k = 1; targets behind the blob's
  // records and draws.  The picks: the argmax's device copy, or the pick's ids
  // output itself -- pinned under do_sample, ids_d with a result copy)
  ffmi_status enqueue_logprobs(const Step &step) {
    const int k = step.k;
    FFMI_CHECK(k == 1 && lp_ws, FFMI_ERR_INVALID);
    const int32_t *picks = result_copy ? ids_d
                           : sampling  ? slot_ids_h(step.slot)
                                       : lp_picks;
    return ffmi_token_logprobs(logits, step.T, c.vocab_size, sampling ? temperature : 0.f,
                               reinterpret_cast<const int32_t *>(step.batch->dev + step_targets.off),
                               picks, lp_h, lp_ws, lp_ws_bytes, (ffmi_stream)stream);
  }

  ffmi_status run_inc(const BatchConfig &bc, InferenceResult *ir) override {
    if (mode != FFMI_MODEL_INC) return FFMI_ERR_INVALID;
    FFMI_CHECK(bc.num_tokens <= o.max_tokens, FFMI_ERR_INVALID);
    pack_inc(bc, o.max_requests, slots, &ps);
    if (sampling) draw_step_u(bc);
    if (logprobs) take_step_targets(bc);
    if (lora) take_step_slots(bc);
    TRY(forward(1));
    memcpy(ir->token_ids, ids_h, bc.num_tokens * sizeof(int32_t));
    if (logprobs) memcpy(ir->logprobs, lp_h, bc.num_tokens * sizeof(float));
    return FFMI_OK;
  }
  ffmi_status run_tree(const TreeVerifyBatchConfig &bc, InferenceResult *ir) override {
    if (mode != FFMI_MODEL_TREE) return FFMI_ERR_INVALID;
    FFMI_CHECK(bc.num_tokens <= o.max_tokens, FFMI_ERR_INVALID);
    pack_tree(bc, o.max_requests, slots, &ps);
    if (logprobs) take_step_targets(bc);
    if (lora) take_step_slots(bc);
    TRY(forward(1));
    memcpy(ir->token_ids, ids_h, bc.num_tokens * sizeof(int32_t));
    if (logprobs) memcpy(ir->logprobs, lp_h, bc.num_tokens * sizeof(float));
    return FFMI_OK;
  }
  ffmi_status run_beam(const BeamSearchBatchConfig &bc, BeamInferenceResult *ir) override {
    TRY(beam_launch(bc));
    return beam_collect(ir);
  }
  ffmi_status beam_launch(const BeamSearchBatchConfig &bc) override {
    return beam_launch_chained(bc, 0);
  }
  ffmi_status beam_collect(BeamInferenceResult *ir) override { return beam_collect_chained(0, ir); }
  // an unsharded SSM, not under debug capture
  bool can_chain_beam() const override {
    return chain_ok && mode == FFMI_MODEL_BEAM && o.tp_size == 1 && !dbg && !result_copy;
  }
  ffmi_status beam_launch_chained(const BeamSearchBatchConfig &bc, int slot) override {
    if (mode != FFMI_MODEL_BEAM) return FFMI_ERR_INVALID;
    FFMI_CHECK(bc.num_tokens <= o.max_tokens && slot >= 0 && slot < kChain, FFMI_ERR_INVALID);
    FFMI_CHECK(slot == 0 || can_chain_beam(), FFMI_ERR_INVALID);
    FFMI_CHECK(chain_batch[slot], FFMI_ERR_INVALID);
    pack_beam(bc, o.max_requests, slots, &ps);
    // a chained step's -1 - i (scheduler entry i of the previous slot) ->
    // -1 - its [T][k] index, which the gather reads from device memory
    for (auto &ti : ps.tokens)
      if (ti.token_id < 0) {
        const long i = -1L - ti.token_id;
        FFMI_CHECK(slot > 0 && i < (long)slot_map[slot - 1].size(), FFMI_ERR_INVALID);
        ti.token_id = -1 - slot_map[slot - 1][i];
      }
    const int k = ps.topk;
    if (step_timing && slot == 0) {
      if (!chain_t0) FFMI_HIP(hipEventCreate(&chain_t0));
      FFMI_HIP(hipEventRecord(chain_t0, stream));
    }
    slot_results[slot] = (size_t)bc.num_tokens * k;
    beam_result_layout(bc, &slot_map[slot]);
    // grouped (chain_group): slots 1 .. kChain-2 staged, launched g at a time
    // (graphed shapes only; anything else first launches what is staged)
    const int Ts = (int)ps.tokens.size();
    const bool grp = chain_group >= 2 && slot >= 1 && slot <= kChain - 2 && use_graphs && !dbg &&
                     prof_level == 0 && Ts > 0 && Ts <= 64;
    ffmi_status st;
    if (grp) {
      st = stage_pending(k, slot);
      if (st == FFMI_OK && ((slot - 1) % chain_group == chain_group - 1 || slot == kChain - 2))
        st = flush_pending();
    } else {
      st = flush_pending();
      if (st == FFMI_OK) st = forward_launch(k, slot);
    }
    // Events let the scheduler replay slot d's bookkeeping while later slots
    // run.  One behind every slot cost the GPU more than the replay it
    // overlapped (same-box A/B, tokens/s: 1333 with, 1342 with none, 1326
    // stepwise); FFMI_CHAIN_EVENTS: 0 none (the collect waits for the whole
    // chain), 1 every slot, 2 (default) one, behind the second-to-last slot:
    // the replays of slots 0 .. D-2 then run while slot D-1 computes
    static const int slot_events =
        getenv("FFMI_CHAIN_EVENTS") ? atoi(getenv("FFMI_CHAIN_EVENTS")) : 2;
    const bool record = slot_events == 1 || (slot_events == 2 && slot == kChain - 2);
    if (st == FFMI_OK) last_slot = slot;
    if (st == FFMI_OK && record) {
      // (so that the scheduler can collect this slot while later ones run)
      if (!slot_ev[slot])
        FFMI_HIP(hipEventCreateWithFlags(&slot_ev[slot], step_timing ? 0 : hipEventDisableTiming));
      FFMI_HIP(hipEventRecord(slot_ev[slot], stream));
      slot_ev_live[slot] = true;
    }
    return st;
  }
  ffmi_status beam_collect_chained(int slot, BeamInferenceResult *ir) override {
    FFMI_CHECK(slot >= 0 && slot < kChain, FFMI_ERR_INVALID);
    TRY(flush_pending());  // (grouped slots still staged go out first)
    int ev = -1;  // the first live event at or after this slot, before the last
    for (int e = slot; e < last_slot && ev < 0; ++e)
      if (slot_ev_live[e] && slot_ev[e]) ev = e;
    if (ev >= 0) {
      // later slots still run: wait for this one (and those before it) only
      FFMI_HIP(hipEventSynchronize(slot_ev[ev]));
    } else {
      const int ls = last_slot;
      TRY(forward_finish());  // (every launched step: one stream)
      for (bool &b : slot_ev_live) b = false;
      // FFMI_STEP_TIMING: the GPU span of a whole chain, from the event before
      // slot 0's launch to the one after the last slot
      if (step_timing && ls > 0 && chain_t0) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, chain_t0, slot_ev[ls]) == hipSuccess) {
          StepTime &q = st_sum[-(ls + 1)];
          q.n++;
          q.gpu += ms * 1e3;
        }
      }
      last_slot = -1;
    }
    const size_t n = slot_results[slot];
    const int32_t *ids = slot_ids_h(slot);
    const float *pr = reinterpret_cast<const float *>(ids + n);
    const std::vector<int> &map = slot_map[slot];
    for (size_t i = 0; i < map.size(); ++i) {
      ir->token_ids[i] = ids[map[i]];
      ir->probs[i] = pr[map[i]];
      ir->parent_id[i] = 0;
    }
    return FFMI_OK;
  }
};

}  // namespace

ffmi_status create_llama_gpu(const ffmi_llama_config *cfg, const ffmi_model_opts *o,
                             ffmi_model **out, unsigned flags) {
  FFMI_CHECK(cfg && o && out, FFMI_ERR_INVALID);
  FFMI_CHECK(o->tp_size >= 1 && o->tp_rank >= 0 && o->tp_rank < o->tp_size, FFMI_ERR_INVALID);
  FFMI_CHECK(o->tp_size == 1 || o->comm, FFMI_ERR_INVALID);
  FFMI_CHECK(o->max_tokens > 0 && o->max_tokens <= BatchConfig::MAX_NUM_TOKENS, FFMI_ERR_INVALID);
  FFMI_CHECK(o->max_requests > 0 && o->max_requests <= BatchConfig::MAX_NUM_REQUESTS,
             FFMI_ERR_INVALID);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return FFMI_ERR_NO_DEVICE;
  LlamaGPU *m = new LlamaGPU();
  m->mode = o->mode;
  m->c = *cfg;
  m->o = *o;
  m->native_gqa = (flags & FFMI_MODEL_NATIVE_GQA) != 0;
  m->lora = (flags & FFMI_MODEL_LORA) != 0;
  if (m->lora && (o->mode == FFMI_MODEL_BEAM || o->tp_size > 1)) {
    delete m;
    ffmi_set_last_error("lora: INC / TREE models at tp_size 1", __FILE__, __LINE__);
    return FFMI_ERR_UNSUPPORTED;
  }
  if (o->weights_folder && o->weights_folder[0]) m->weights_folder = o->weights_folder;
  m->o.weights_folder = nullptr;
  ffmi_status st = m->init();
  if (st != FFMI_OK) {
    delete m;
    return st;
  }
  *out = m;
  return FFMI_OK;
}

}  // namespace ffmi
