// Stand-alone driver of the host-side transfer planner
// (csrc/sem_transfer_plan.cpp): launches no kernel and needs no GPU
// (tests/test_transfer_host.py).  It links the planner and the host basis
// tables it calls (csrc/sem_basis.cpp: sem_gll_table, sem_lagrange_eval).
// One JSON line on stdout per call:
//   transfer_check matrix <p_from> <p_to>      J [n_to][n_from], row-major
//   transfer_check matrices                    J of all 256 order pairs
//   transfer_check plan <ndim> <p_from> <p_to> <n_elem> <from.bin>
//                       <n_node_from> <to.bin> <n_node_to>
//                                              validation of the two uint32
//                                              maps, then the owner mask and
//                                              the "from" node CSR
//   hipcc -std=c++17 -Ispectralelementmethod_amd/csrc tools/transfer_check.cpp \
//       spectralelementmethod_amd/csrc/sem_transfer_plan.cpp \
//       spectralelementmethod_amd/csrc/sem_basis.cpp -o transfer_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sem_transfer_plan.h"

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

void print_doubles(const char* key, const std::vector<double>& v, const char* tail) {
  std::printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("]%s", tail);
}

int refused(int rc) {
  std::printf("{\"rc\": %d, \"error\": \"", rc);
  for (const char* c = sem_last_error(); *c; ++c) {
    if (*c == '"' || *c == '\\') std::putchar('\\');
    std::putchar(*c);
  }
  std::printf("\"}\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "matrix")) {
    std::vector<double> J, Jt;
    const int rc = semtransfer::interp_matrix(std::atoi(argv[2]), std::atoi(argv[3]), J, Jt);
    if (rc != SEM_OK) return refused(rc);
    std::printf("{\"rc\": 0, ");
    print_doubles("J", J, ", ");
    print_doubles("Jt", Jt, "}\n");
    return 0;
  }
  if (argc == 2 && !std::strcmp(argv[1], "matrices")) {
    std::printf("{\"pairs\": [");
    for (int pf = 1; pf <= 16; ++pf)
      for (int pt = 1; pt <= 16; ++pt) {
        std::vector<double> J, Jt;
        if (semtransfer::interp_matrix(pf, pt, J, Jt) != SEM_OK) return 2;
        std::printf("%s{\"p_from\": %d, \"p_to\": %d, ", pf + pt > 2 ? ", " : "", pf, pt);
        print_doubles("J", J, "}");
      }
    std::printf("]}\n");
    return 0;
  }
  if (argc == 10 && !std::strcmp(argv[1], "plan")) {
    const int ndim = std::atoi(argv[2]), p_from = std::atoi(argv[3]), p_to = std::atoi(argv[4]);
    const int64_t n_elem = std::atoll(argv[5]);
    const int64_t n_node_from = std::atoll(argv[7]), n_node_to = std::atoll(argv[9]);
    int rc = semtransfer::check_sizes(ndim, p_from, p_to, n_elem, n_node_from, n_node_to);
    if (rc != SEM_OK) return refused(rc);
    const std::vector<uint32_t> from = read_file(argv[6]), to = read_file(argv[8]);
    int64_t nloc_from = 1, nloc_to = 1;
    for (int i = 0; i < ndim; ++i) {
      nloc_from *= p_from + 1;
      nloc_to *= p_to + 1;
    }
    if ((int64_t)from.size() != n_elem * nloc_from || (int64_t)to.size() != n_elem * nloc_to) {
      std::fprintf(stderr, "map files do not hold n_elem * n^ndim entries\n");
      return 2;
    }
    rc = semtransfer::check_map("from", from.data(), (int64_t)from.size(), n_node_from);
    if (rc == SEM_OK) rc = semtransfer::check_map("to", to.data(), (int64_t)to.size(), n_node_to);
    if (rc != SEM_OK) return refused(rc);
    semtransfer::Plan pl;
    semtransfer::plan((int64_t)from.size(), from.data(), n_node_from, (int64_t)to.size(),
                      to.data(), n_node_to, pl);
    std::printf("{\"rc\": 0, \"error\": \"\", ");
    print_list("owner", pl.owner, ", ");
    print_list("ptr", pl.ptr, ", ");
    print_list("entry", pl.entry, ", ");
    std::printf("\"n_owned\": %lld, \"max_row\": %lld}\n", (long long)pl.n_owned,
                (long long)pl.max_row);
    return 0;
  }
  std::fprintf(stderr, "usage: transfer_check matrix|matrices|plan ...\n");
  return 2;
}
