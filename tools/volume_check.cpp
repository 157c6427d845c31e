// Stand-alone driver of the host-side volume planner
// (csrc/sem_volume_plan.cpp): launches no kernel and needs no GPU
// (tests/test_volume_host.py).  One JSON line on stdout per call:
//   volume_check plan <ndim> <p> <n_elem> <e2n.bin> <n_node>
//                         validation of the sizes and of the uint32 map, then
//                         the CSR of the (element, local) entries of every node
//   hipcc -std=c++17 -Ispectralelementmethod_amd/csrc tools/volume_check.cpp \
//       spectralelementmethod_amd/csrc/sem_volume_plan.cpp -o volume_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sem_volume_plan.h"

// the planner reports through sem::fail (csrc/sem_error.h), which the library
// keeps in csrc/sem_basis.cpp: this driver links without it
namespace {
std::string g_error;
}
namespace sem {
int fail(int code, const std::string& msg) {
  g_error = msg;
  return code;
}
}  // namespace sem

namespace {

std::vector<uint32_t> read_file(const char* path) {
  std::vector<uint32_t> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(2);
  }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / sizeof(uint32_t));
  if (!v.empty() && std::fread(v.data(), sizeof(uint32_t), v.size(), f) != v.size()) std::exit(2);
  std::fclose(f);
  return v;
}

template <class V>
void print_list(const char* key, const V& v, const char* tail) {
  std::printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? ", " : "", (long long)v[i]);
  std::printf("]%s", tail);
}

int refused(int rc) {
  std::printf("{\"rc\": %d, \"error\": \"", rc);
  for (const char* c = g_error.c_str(); *c; ++c) {
    if (*c == '"' || *c == '\\') std::putchar('\\');
    std::putchar(*c);
  }
  std::printf("\"}\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 7 && !std::strcmp(argv[1], "plan")) {
    const int ndim = std::atoi(argv[2]), p = std::atoi(argv[3]);
    const int64_t n_elem = std::atoll(argv[4]), n_node = std::atoll(argv[6]);
    int rc = semvolume::check_sizes(ndim, p, n_elem, n_node);
    if (rc != SEM_OK) return refused(rc);
    const std::vector<uint32_t> map = read_file(argv[5]);
    int64_t nloc = 1;
    for (int i = 0; i < ndim; ++i) nloc *= p + 1;
    if ((int64_t)map.size() != n_elem * nloc) {
      std::fprintf(stderr, "the map file does not hold n_elem * n^ndim entries\n");
      return 2;
    }
    rc = semvolume::check_map(map.data(), (int64_t)map.size(), n_node);
    if (rc != SEM_OK) return refused(rc);
    semvolume::Plan pl;
    semvolume::plan((int64_t)map.size(), map.data(), n_node, pl);
    std::printf("{\"rc\": 0, \"error\": \"\", ");
    print_list("ptr", pl.ptr, ", ");
    print_list("entry", pl.entry, ", ");
    std::printf("\"n_referenced\": %lld, \"max_row\": %lld}\n", (long long)pl.n_referenced,
                (long long)pl.max_row);
    return 0;
  }
  std::fprintf(stderr, "usage: volume_check plan <ndim> <p> <n_elem> <e2n.bin> <n_node>\n");
  return 2;
}
