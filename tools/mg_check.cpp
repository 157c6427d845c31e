// Stand-alone driver of the host-side p-multigrid planner
// (csrc/sem_mg_plan.cpp): launches no kernel and needs no GPU
// (tests/test_mg_host.py).  It links the planner and the unit that holds the
// error message (csrc/sem_basis.cpp).  One JSON line on stdout per call:
//   mg_check ladders                      the default ladder of p = 0 .. 17
//   mg_check ladder <p0> <p1> ...         check_ladder of a caller's chain
//   mg_check coarsen <ndim> <p_fine> <p_coarse> <n_elem> <fine.bin>
//                    <n_node_fine> <mask.bin>
//                                         the coarse map, the kept fine ids
//                                         and the coarse mask of a uint32 map
//                                         and a uint8 mask
//   mg_check cheb <degree> <lambda_max> <ratio>
//                                         inv_theta, c1, c2
//   mg_check counts <n_levels> <k> <kc>   actions and passes per level
//   mg_check create                       check_create / check_level_sizes on
//                                         a table of bad arguments
//   hipcc -std=c++17 -Ispectralelementmethod_amd/csrc tools/mg_check.cpp \
//       spectralelementmethod_amd/csrc/sem_mg_plan.cpp \
//       spectralelementmethod_amd/csrc/sem_basis.cpp -o mg_check
// (add -fsanitize=address,undefined for a sanitised run on the CPU)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sem_mg_plan.h"

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

void print_doubles(const char* key, const std::vector<double>& v, const char* tail) {
  std::printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("]%s", tail);
}

void print_error() {
  std::printf("\"error\": \"");
  for (const char* c = sem_last_error(); *c; ++c) {
    if (*c == '"' || *c == '\\') std::putchar('\\');
    std::putchar(*c);
  }
  std::printf("\"");
}

int refused(int rc) {
  std::printf("{\"rc\": %d, ", rc);
  print_error();
  std::printf("}\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "ladders")) {
    std::printf("{\"ladders\": [");
    for (int p = 0; p <= 17; ++p) {
      std::vector<int> lad;
      const int rc = semmg::default_ladder(p, lad);
      std::printf("%s{\"p\": %d, \"rc\": %d, ", p ? ", " : "", p, rc);
      print_list("ladder", lad, "}");
    }
    std::printf("]}\n");
    return 0;
  }
  if (argc >= 2 && !std::strcmp(argv[1], "ladder")) {
    std::vector<int> lad;
    for (int i = 2; i < argc; ++i) lad.push_back(std::atoi(argv[i]));
    return refused(semmg::check_ladder(lad.empty() ? nullptr : lad.data(), (int)lad.size()));
  }
  if (argc == 9 && !std::strcmp(argv[1], "coarsen")) {
    const int ndim = std::atoi(argv[2]), pf = std::atoi(argv[3]), pc = std::atoi(argv[4]);
    const int64_t n_elem = std::atoll(argv[5]), n_node = std::atoll(argv[7]);
    int rc = semmg::check_coarsen(ndim, pf, pc, n_elem, n_node);
    if (rc != SEM_OK) return refused(rc);
    const std::vector<uint32_t> fine = read_file<uint32_t>(argv[6]);
    const std::vector<uint8_t> mask = read_file<uint8_t>(argv[8]);
    int64_t nloc = 1;
    for (int i = 0; i < ndim; ++i) nloc *= pf + 1;
    if ((int64_t)fine.size() != n_elem * nloc || (int64_t)mask.size() != n_node) {
      std::fprintf(stderr, "the files do not hold n_elem * n^ndim ids and n_node flags\n");
      return 2;
    }
    std::vector<uint32_t> coarse, keep;
    rc = semmg::coarsen(ndim, pf, pc, n_elem, fine.data(), n_node, coarse, keep);
    if (rc != SEM_OK) return refused(rc);
    std::vector<uint8_t> mc;
    rc = semmg::coarse_mask(ndim, pf, pc, n_elem, fine.data(), n_node, mask.data(), coarse.data(),
                            (int64_t)keep.size(), mc);
    if (rc != SEM_OK) return refused(rc);
    std::printf("{\"rc\": 0, \"error\": \"\", ");
    print_list("e2n_coarse", coarse, ", ");
    print_list("keep", keep, ", ");
    print_list("mask_coarse", mc, "}\n");
    return 0;
  }
  if (argc == 5 && !std::strcmp(argv[1], "cheb")) {
    semmg::Cheb c;
    const int rc = semmg::chebyshev(std::atoi(argv[2]), std::atof(argv[3]), std::atof(argv[4]), c);
    if (rc != SEM_OK) return refused(rc);
    std::printf("{\"rc\": 0, \"inv_theta\": %.17g, ", c.inv_theta);
    print_doubles("c1", c.c1, ", ");
    print_doubles("c2", c.c2, "}\n");
    return 0;
  }
  if (argc == 5 && !std::strcmp(argv[1], "counts")) {
    std::vector<int> actions, passes;
    semmg::cycle_counts(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), actions,
                        passes);
    std::printf("{");
    print_list("actions", actions, ", ");
    print_list("passes", passes, "}\n");
    return 0;
  }
  if (argc == 2 && !std::strcmp(argv[1], "create")) {
    // stand-ins for the handles: check_create looks only at NULL / not NULL
    int dummy = 0;
    const void* ok3[3] = {&dummy, &dummy, &dummy};
    const void* hole3[3] = {&dummy, nullptr, &dummy};
    const double lam[3] = {2.3, 2.1, 1.9}, lam_bad[3] = {2.3, -1.0, 1.9};
    const double lam_nan[3] = {2.3, 2.1, std::atof("nan")};
    struct Case {
      const char* name;
      int rc;
    };
    std::vector<Case> out;
    auto run = [&](const char* name, int n, const void* const* c, const void* const* t,
                   const void* const* m, const double* l, int k, int kc, double ratio,
                   double cratio) {
      out.push_back({name, semmg::check_create(n, c, t, m, l, k, kc, ratio, cratio)});
    };
    run("ok", 3, ok3, ok3, ok3, lam, 2, 8, 4.0, 30.0);
    run("one_level_no_transfers", 1, ok3, nullptr, ok3, lam, 2, 8, 4.0, 30.0);
    run("no_levels", 0, ok3, ok3, ok3, lam, 2, 8, 4.0, 30.0);
    run("too_many_levels", 17, ok3, ok3, ok3, lam, 2, 8, 4.0, 30.0);
    run("null_ctxs", 3, nullptr, ok3, ok3, lam, 2, 8, 4.0, 30.0);
    run("null_transfers", 3, ok3, nullptr, ok3, lam, 2, 8, 4.0, 30.0);
    run("null_masks", 3, ok3, ok3, nullptr, lam, 2, 8, 4.0, 30.0);
    run("null_lambda", 3, ok3, ok3, ok3, nullptr, 2, 8, 4.0, 30.0);
    run("null_ctx_entry", 3, hole3, ok3, ok3, lam, 2, 8, 4.0, 30.0);
    run("null_transfer_entry", 3, ok3, hole3, ok3, lam, 2, 8, 4.0, 30.0);
    run("null_mask_entry", 3, ok3, ok3, hole3, lam, 2, 8, 4.0, 30.0);
    run("negative_lambda", 3, ok3, ok3, ok3, lam_bad, 2, 8, 4.0, 30.0);
    run("nan_lambda", 3, ok3, ok3, ok3, lam_nan, 2, 8, 4.0, 30.0);
    run("smooth_degree_0", 3, ok3, ok3, ok3, lam, 0, 8, 4.0, 30.0);
    run("coarse_degree_0", 3, ok3, ok3, ok3, lam, 2, 0, 4.0, 30.0);
    run("smooth_ratio_1", 3, ok3, ok3, ok3, lam, 2, 8, 1.0, 30.0);
    run("coarse_ratio_below_1", 3, ok3, ok3, ok3, lam, 2, 8, 4.0, 0.5);
    out.push_back({"sizes_ok", semmg::check_level_sizes(0, 289, 81, 81, 289)});
    out.push_back({"sizes_fine_mismatch", semmg::check_level_sizes(0, 288, 81, 81, 289)});
    out.push_back({"sizes_coarse_mismatch", semmg::check_level_sizes(1, 289, 81, 80, 289)});
    std::printf("{");
    for (size_t i = 0; i < out.size(); ++i)
      std::printf("%s\"%s\": %d", i ? ", " : "", out[i].name, out[i].rc);
    std::printf("}\n");
    return 0;
  }
  std::fprintf(stderr, "usage: mg_check ladders|ladder|coarsen|cheb|counts|create ...\n");
  return 2;
}
