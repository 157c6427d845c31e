// Stand-alone driver of the host-side face planner (csrc/sem_faces_plan.cpp):
// links no HIP and needs no GPU (tests/test_faces_host.py).  One JSON line on
// stdout per call:
//   faces_check tables <ndim> <n>                  the face-order index tables
//   faces_check csr <nodes.bin>                    the node CSR of uint32 node
//                                                  ids, one per (face, q) entry
//   faces_check check <ndim> <p> <n_elem> <elem.bin> <face.bin>
//                                                  validation of int32 element
//                                                  and uint8 face ids
//   g++ -std=c++17 -Ispectralelementmethod_amd/csrc tools/faces_check.cpp \
//       spectralelementmethod_amd/csrc/sem_faces_plan.cpp -o faces_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sem_error.h"
#include "sem_faces_plan.h"

namespace {
std::string g_error;
}

namespace sem {
void set_error(const std::string& msg) { g_error = msg; }
int fail(int code, const std::string& msg) {
  g_error = msg;
  return code;
}
}  // namespace sem

namespace {

template <class T>
std::vector<T> read_file(const char* path) {
  std::vector<T> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(2);
  }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / sizeof(T));
  if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(2);
  std::fclose(f);
  return v;
}

template <class V>
void print_list(const char* key, const V& v, const char* tail) {
  std::printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? ", " : "", (long long)v[i]);
  std::printf("]%s", tail);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "tables")) {
    const int ndim = std::atoi(argv[2]), n = std::atoi(argv[3]);
    if ((ndim != 2 && ndim != 3) || n < 2 || n > 17) return 2;
    std::vector<int32_t> t;
    semfaces::index_tables(ndim, n, t);
    std::printf("{");
    print_list("table", t, "}\n");
    return 0;
  }
  if (argc == 3 && !std::strcmp(argv[1], "csr")) {
    const std::vector<uint32_t> node = read_file<uint32_t>(argv[2]);
    semfaces::NodeCsr csr;
    semfaces::node_csr(node.data(), (int64_t)node.size(), csr);
    std::printf("{");
    print_list("node", csr.node, ", ");
    print_list("ptr", csr.ptr, ", ");
    print_list("entry", csr.entry, ", ");
    std::printf("\"max_row\": %lld}\n", (long long)csr.max_row);
    return 0;
  }
  if (argc == 7 && !std::strcmp(argv[1], "check")) {
    const std::vector<int32_t> elem = read_file<int32_t>(argv[5]);
    const std::vector<uint8_t> face = read_file<uint8_t>(argv[6]);
    if (elem.size() != face.size()) return 2;
    const int rc = semfaces::check(std::atoi(argv[2]), std::atoi(argv[3]), std::atoll(argv[4]),
                                   (int64_t)elem.size(), elem.data(), face.data());
    std::printf("{\"rc\": %d, \"error\": \"%s\"}\n", rc, rc ? g_error.c_str() : "");
    return 0;
  }
  std::fprintf(stderr, "usage: faces_check tables|csr|check ...\n");
  return 2;
}
