// tensor_file.cpp -- see tensor_file.h.
#include "tensor_file.h"

#include <stdio.h>

#include <algorithm>

namespace ffmi {

namespace {

inline void convert(float v, uint16_t *out) {  // round to nearest even
  const _Float16 h = (_Float16)v;
  memcpy(out, &h, 2);
}
inline void convert(uint16_t bits, float *out) {
  _Float16 h;
  memcpy(&h, &bits, 2);
  *out = (float)h;
}

// n elements of type Out: the file holds them as they are, or as Other (by
// its size), converted a block at a time
template <typename Other, typename Out>
TensorRead read_as(const std::string &path, size_t n, Out *dst) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return TensorRead::not_found;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  bool ok = false;
  if (bytes == (long)(n * sizeof(Out))) {
    ok = fread(dst, sizeof(Out), n, f) == n;
  } else if (bytes == (long)(n * sizeof(Other))) {
    Other block[2048];
    const size_t cap = sizeof(block) / sizeof(Other);
    ok = true;
    for (size_t i = 0; ok && i < n; i += cap) {
      const size_t m = std::min(cap, n - i);
      ok = fread(block, sizeof(Other), m, f) == m;
      for (size_t j = 0; ok && j < m; ++j) convert(block[j], &dst[i + j]);
    }
  }
  fclose(f);
  return ok ? TensorRead::ok : TensorRead::wrong_size;
}

}  // namespace

TensorRead read_tensor(const std::string &path, size_t n, uint16_t *dst) {
  return read_as<float>(path, n, dst);
}
TensorRead read_tensor(const std::string &path, size_t n, float *dst) {
  return read_as<uint16_t>(path, n, dst);
}

}  // namespace ffmi
