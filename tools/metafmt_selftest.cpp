// Stand-alone check of the device metadata formatter's host instance (csrc/common/metafmt.h)
// against the host formatters it must reproduce (csrc/host/rustfmt.h). Built by
// tests/test_device_meta.py with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/metafmt_selftest.cpp -o metafmt_selftest
//   ./metafmt_selftest [case.bin ...]
//
//  * {:.2} and {:.4} of every double quotient a / b, 0 <= a <= 2000, 1 <= b <= 2000, against
//    append_fixed;
//  * 200,000 seeded doubles in [0.2, 1] (and the doubles next to the confidences 1 / den) against
//    append_f64;
//  * for every case file (the record matrices of tests/meta_matrix.py, written by the test): the
//    size sink and the write sink report the same length for every row, the write sink fills an
//    exactly sized heap buffer (so an overrun is an AddressSanitizer error), and the lengths equal
//    the offsets the test recorded.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../csrc/common/metafmt.h"
#include "../csrc/host/rustfmt.h"

using namespace tb;

struct StrSink {
  std::string s;
  void put(char c) { s.push_back(c); }
  void copy(const char* p, uint32_t n) { s.append(p, n); }
};

static int g_bad = 0;

static void check(const std::string& got, const std::string& want, const char* what, double x) {
  if (got == want) return;
  if (++g_bad <= 20) std::fprintf(stderr, "%s(%.17g): got '%s' want '%s'\n", what, x, got.c_str(), want.c_str());
}

static void check_fixed(double x) {
  for (int prec : {2, 4}) {
    StrSink k;
    MetaCountSink c;
    const bool ok = meta_fixed(k, x, prec);
    meta_fixed(c, x, prec);
    std::string want;
    append_fixed(want, x, prec);
    if (!ok) k.s = "<unformattable>";
    check(k.s, want, prec == 2 ? "fixed2" : "fixed4", x);
    if (c.n != k.s.size()) check("count " + std::to_string(c.n), "count " + std::to_string(k.s.size()), "fixed", x);
  }
}

static void check_f64(double x) {
  StrSink k;
  MetaCountSink c;
  const bool ok = meta_f64(k, x);
  meta_f64(c, x);
  std::string want;
  append_f64(want, x);
  if (!ok) k.s = "<unformattable>";
  check(k.s, want, "f64", x);
  if (c.n != k.s.size()) check("count " + std::to_string(c.n), "count " + std::to_string(k.s.size()), "f64", x);
}

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

// case file: int64 {ndocs, nrecs, nk, nx, ntok}, DevResolve, DevMetaPlan, per record buffer int64 length +
// values, fail int32 [ndocs], rows int32 [nk + nx], ntok x tokens int32 [nk], offsets int64 [nk + nx + 1]
static bool check_case(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  int64_t hd[5];
  auto rp = std::make_unique<DevResolve>();
  auto mp = std::make_unique<DevMetaPlan>();
  bool ok = std::fread(hd, sizeof(int64_t), 5, f) == 5 && std::fread(rp.get(), sizeof(DevResolve), 1, f) == 1 &&
            std::fread(mp.get(), sizeof(DevMetaPlan), 1, f) == 1;
  if (!ok) { std::fclose(f); return false; }
  const int64_t ndocs = hd[0], nrecs = hd[1], nk = hd[2], nx = hd[3], ntok = hd[4];
  std::vector<std::vector<int64_t>> recs((size_t)nrecs);
  for (auto& r : recs) {
    int64_t len = 0;
    ok = ok && std::fread(&len, sizeof(len), 1, f) == 1 && read_vec(f, r, (size_t)len);
  }
  std::vector<int32_t> fail, rows;
  std::vector<std::vector<int32_t>> toks((size_t)ntok);
  std::vector<int64_t> off;
  ok = ok && read_vec(f, fail, (size_t)ndocs) && read_vec(f, rows, (size_t)(nk + nx));
  for (auto& t : toks) ok = ok && read_vec(f, t, (size_t)nk);
  ok = ok && read_vec(f, off, (size_t)(nk + nx + 1));
  std::fclose(f);
  if (!ok || ntok != mp->n_tokens) return false;
  std::vector<const int64_t*> rptr;
  for (auto& r : recs) rptr.push_back(r.data());
  for (int64_t pos = 0; pos < nk + nx; ++pos) {
    int32_t tok[kMaxMetaTokens] = {0};
    for (int64_t t = 0; t < ntok; ++t) tok[t] = pos < nk ? toks[(size_t)t][(size_t)pos] : -1;
    const int32_t fl = pos < nk ? -1 : fail[(size_t)rows[(size_t)pos]];
    MetaCountSink c;
    const bool ok_c = meta_row(*rp, *mp, rptr.data(), ndocs, rows[(size_t)pos], fl, tok, c);
    std::unique_ptr<char[]> buf(new char[c.n ? c.n : 1]);  // exactly sized: ASan sees an overrun
    MetaWriteSink w(buf.get());
    const bool ok_w = meta_row(*rp, *mp, rptr.data(), ndocs, rows[(size_t)pos], fl, tok, w);
    if (c.n != w.n || ok_c != ok_w || (int64_t)c.n != off[(size_t)pos + 1] - off[(size_t)pos]) {
      if (++g_bad <= 20)
        std::fprintf(stderr, "%s row %lld: size pass %u, write pass %u, recorded %lld\n", path, (long long)pos, c.n,
                     w.n, (long long)(off[(size_t)pos + 1] - off[(size_t)pos]));
    }
  }
  return true;
}

int main(int argc, char** argv) {
  long n_fixed = 0, n_f64 = 0;
  for (int a = 0; a <= 2000; ++a)
    for (int b = 1; b <= 2000; ++b, ++n_fixed) check_fixed((double)a / (double)b);
  for (double x : {0.0, 1e-300, 4.9e-324, 0.005, 0.015, 0.125, 3.125, 99999.995, 1e6 + 0.125, 1099511627776.5,
                   99999999999999.0, -0.125, -2.5})
    check_fixed(x);
  std::mt19937_64 rng(20240611);
  std::uniform_real_distribution<double> uni(0.2, 1.0);
  for (int i = 0; i < 200000; ++i, ++n_f64) check_f64(uni(rng));
  for (int den = 1; den <= 5; ++den) {
    const double v = 1.0 / den;
    for (double x : {v, std::nextafter(v, 0.0), std::nextafter(v, 2.0)}) check_f64(x);
  }
  for (double x : {0.9999999999999999, 0.125, 1.5, 1.9999999999999998, 0.3, 0.7, 0.65}) check_f64(x);
  {  // outside the supported range: refused, never approximated
    StrSink k;
    if (meta_f64(k, 2.0) || meta_f64(k, 0.1) || meta_f64(k, std::nan("")) || meta_fixed(k, 1e14, 2) ||
        meta_fixed(k, INFINITY, 4) || !k.s.empty()) {
      std::fprintf(stderr, "an out-of-range value was formatted\n");
      ++g_bad;
    }
  }
  int n_cases = 0;
  for (int i = 1; i < argc; ++i) {
    if (!check_case(argv[i])) {
      std::fprintf(stderr, "%s: unreadable case file\n", argv[i]);
      ++g_bad;
    }
    ++n_cases;
  }
  std::printf("metafmt_selftest: %ld quotients x 2 precisions, %ld doubles, %d case files, %d mismatches\n", n_fixed,
              n_f64, n_cases, g_bad);
  return g_bad ? 1 : 0;
}
