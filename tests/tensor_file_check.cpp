// tensor_file_check.cpp -- drives runtime/tensor_file.{h,cpp} for
// tests/test_tensor_file_host.py (host build under the address and
// undefined-behaviour sanitizers).
//   f16 | f32 <path> <n> <out>   read n elements; prints the outcome, writes
//                                the n elements read to <out>
//   rep16 | rep32 <heads> <kv_heads> <n_src> <in> <out>   K/V row replication
// The read buffer carries guard words behind its n elements: exit 3 if a
// read touched them.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../flexflow_amd/csrc/runtime/tensor_file.h"

namespace {

constexpr size_t kGuard = 8;

template <typename T>
T guard_word() {
  T g;
  memset(&g, 0xA5, sizeof(T));
  return g;
}

bool write_file(const char *path, const void *p, size_t bytes) {
  FILE *f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(p, 1, bytes, f) == bytes;
  return fclose(f) == 0 && ok;
}

template <typename T>
int run_read(const char *path, size_t n, const char *out) {
  std::vector<T> buf(n + kGuard, guard_word<T>());
  const ffmi::TensorRead r = ffmi::read_tensor(path, n, buf.data());
  const T g = guard_word<T>();
  for (size_t i = n; i < n + kGuard; ++i)
    if (memcmp(&buf[i], &g, sizeof(T)) != 0) {
      printf("guard word %zu overwritten\n", i - n);
      return 3;
    }
  printf("%s\n", r == ffmi::TensorRead::ok          ? "ok"
                 : r == ffmi::TensorRead::not_found ? "not_found"
                                                    : "wrong_size");
  if (r == ffmi::TensorRead::ok && !write_file(out, buf.data(), n * sizeof(T))) return 2;
  return 0;
}

template <typename T>
int run_rep(int heads, int kv_heads, size_t n_src, const char *in, const char *out) {
  std::vector<T> src(n_src), dst(n_src / kv_heads * heads);
  FILE *f = fopen(in, "rb");
  if (!f || fread(src.data(), sizeof(T), n_src, f) != n_src) return 2;
  fclose(f);
  ffmi::replicate_kv_heads(src.data(), n_src, heads, kv_heads, dst.data());
  return write_file(out, dst.data(), dst.size() * sizeof(T)) ? 0 : 2;
}

}  // namespace

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "f16" && argc == 5)
    return run_read<uint16_t>(argv[2], strtoull(argv[3], nullptr, 10), argv[4]);
  if (mode == "f32" && argc == 5)
    return run_read<float>(argv[2], strtoull(argv[3], nullptr, 10), argv[4]);
  const size_t n_src = argc == 7 ? strtoull(argv[4], nullptr, 10) : 0;
  if (mode == "rep16" && argc == 7)
    return run_rep<uint16_t>(atoi(argv[2]), atoi(argv[3]), n_src, argv[5], argv[6]);
  if (mode == "rep32" && argc == 7)
    return run_rep<float>(atoi(argv[2]), atoi(argv[3]), n_src, argv[5], argv[6]);
  fprintf(stderr, "usage: see the head of tensor_file_check.cpp\n");
  return 64;
}
