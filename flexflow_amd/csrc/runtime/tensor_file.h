// tensor_file.h -- the per-tensor files of a reference-format checkpoint or
// adapter folder (file_loader.cc:363-389 load_from_file; convert_hf_model
// writes one raw file per tensor, fp16 or fp32).  Host only: no HIP, no
// last-error state; the callers turn an outcome into their own message.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace ffmi {

enum class TensorRead { ok, not_found, wrong_size };

// n elements of `path` as fp16 bits: a 2n-byte file as it is, a 4n-byte fp32
// file converted with round to nearest even
TensorRead read_tensor(const std::string &path, size_t n, uint16_t *dst);
// ... as fp32: a 4n-byte file as it is, a 2n-byte fp16 file widened (exact)
TensorRead read_tensor(const std::string &path, size_t n, float *dst);

// "<what> not found: <path>" / "<what> has the wrong size: <path>"
inline std::string tensor_read_message(TensorRead r, const char *what, const std::string &path) {
  return what + std::string(r == TensorRead::not_found ? " not found: " : " has the wrong size: ") +
         path;
}

// K/V rows replicated per query head: src [kv_heads * d][H] (n_src elements)
// -> dst [heads * d][H], row block of query head i = kv head
// i / (heads / kv_heads) (file_loader.cc:292-302)
template <typename T>
void replicate_kv_heads(const T *src, size_t n_src, int heads, int kv_heads, T *dst) {
  const size_t row_block = n_src / kv_heads;  // d rows of one head
  const int group = heads / kv_heads;
  for (int i = 0; i < heads; ++i)
    memcpy(dst + (size_t)i * row_block, src + (size_t)(i / group) * row_block,
           row_block * sizeof(T));
}

// The n elements of tensor `hf_name` of the checkpoint in `folder`; *path is
// its file, the HF name without "model." (as convert_hf_model writes them).
// The k/v projections of a GQA checkpoint hold kv_heads * d rows: they are
// replicated to heads * d (pass kv_heads = heads to take them as stored).
template <typename T>
TensorRead read_checkpoint_tensor(const std::string &folder, const std::string &hf_name, size_t n,
                                  int heads, int kv_heads, std::vector<T> *out, std::string *path) {
  const std::string file = hf_name.rfind("model.", 0) == 0 ? hf_name.substr(6) : hf_name;
  const bool kv = file.find("self_attn.k_proj") != std::string::npos ||
                  file.find("self_attn.v_proj") != std::string::npos;
  *path = folder + "/" + file;
  out->resize(n);
  if (!kv || kv_heads == heads) return read_tensor(*path, n, out->data());
  std::vector<T> stored(n / (heads / kv_heads));
  const TensorRead r = read_tensor(*path, stored.size(), stored.data());
  if (r == TensorRead::ok)
    replicate_kv_heads(stored.data(), stored.size(), heads, kv_heads, out->data());
  return r;
}

}  // namespace ffmi
