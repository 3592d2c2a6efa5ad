// K18: the output metadata column ({"gopher_quality_filter_status":"filtered",...}) formatted from
// the device records, one source for the kernels (k_meta_size / k_meta_write) and their host
// emulation. It reproduces what BatchState::assemble builds for a row without input metadata
// (csrc/host/pipeline.cpp: step_meta_json over steps 0..last, filters.cpp decide_t<JsonSink>).
//
// Everything that does not depend on the document is a literal of the plan's string pool, already
// JSON-escaped and with the configured thresholds formatted by the host (build_meta_plan): member
// keys, status values, reason prefixes and suffixes. Per row the formatter only copies literals and
// formats the dynamic values: int64 counts, {:.2} / {:.4} of the double quotient of two record
// fields, and the language confidence (Rust f64 Display). The failing step runs decide_t's branch
// chain in its order, with the double-precision expressions of gate_fails (gate.h).
//
// The formatter is a template over a sink; MetaCountSink and MetaWriteSink run the same code, so
// the size pass and the write pass cannot disagree.
#pragma once
#include "gate.h"

// The value formatters are real calls in the kernels: the branch chains reach them from ~40 places
// and 128-bit arithmetic inlined at each would cost registers for nothing.
#if defined(__HIPCC__)
#define TB_HD_CALL __host__ __device__ __noinline__
#else
#define TB_HD_CALL inline
#endif

namespace tb {

constexpr int kMaxMetaLits = 80;       // literals per step (GopherRepetition: 4 + 2 * (4 + 16 + 16))
constexpr int kMetaPoolBytes = 8192;   // the plan's literal pool
constexpr int kMaxMetaTokens = 4;      // trailing TokenCounter steps
constexpr int kMetaLangs = 5;          // filters.cpp kLangNames

struct MetaLit {
  uint16_t off, len;
};

// literal slots of a step (DevMetaStep::lit)
enum : int32_t {
  ML_PASSED = 0,  // the members of a passing step (len 0: none)
  ML_HEAD = 1,    // multi-reason steps: "x_status":"filtered","x_reasons":"  (the value stays open)
  ML_X0 = 2,      // kind-specific
  ML_X1 = 3,
  ML_REASON0 = 4,  // reason r: prefix ML_REASON0 + 2r, suffix ML_REASON0 + 2r + 1
};
// GopherQuality: ML_X0 = suffix of gopher_below_avg_threshold when the document has no words;
// reasons in decide_t order
enum : int32_t { MQ_SHORT = 0, MQ_LONG, MQ_BELOW_AVG, MQ_ABOVE_AVG, MQ_HASHES, MQ_ELLIPSIS, MQ_BULLETS, MQ_ELL_LINES,
                 MQ_ALPHA, MQ_STOP };
// GopherRepetition: ML_X0 = the complete members of "skipping empty content"; reasons 0..3 the
// four fractions, then the top orders, then the duplicated orders
// C4Quality: ML_X0 / ML_X1 = lorem_ipsum / curly_bracket; reason 0 = too_few_sentences; then the
// three line-filter members (each ,"key":" with the value left open)
enum : int32_t { MC_LINE0 = ML_REASON0 + 2 };
// FineWeb: ML_X0 / ML_X1 = the complete members of "empty document" / list_ratio_no_words;
// reasons 0..3 = line_punct, short_line, char_dup, list_ratio (prefix holds the members' start,
// suffix the closing quote)
// LanguageDetection: ML_X0 + l = "Detected language":"<name l>","Detected language confidence":"

struct DevMetaStep {
  MetaLit lit[kMaxMetaLits];
};

struct DevMetaPlan {
  int32_t n_steps;       // = DevResolve::gate.n_steps (same order)
  int32_t n_tokens;      // trailing TokenCounter steps (kept rows: "token_count":"N" each)
  int32_t row_cap;       // output bytes the column buffer holds per output row (see build_meta_plan)
  int32_t pool_used;
  MetaLit token;         // "token_count":"
  MetaLit pad;
  DevMetaStep steps[kMaxGateSteps];
  char pool[kMetaPoolBytes];
};

// error word bits of a formatted batch
constexpr int32_t kMetaErrOverflow = 1;      // the column does not fit row_cap * rows
constexpr int32_t kMetaErrUnformattable = 2;  // a value outside what the formatter reproduces exactly

struct MetaCountSink {
  uint32_t n = 0;
  TB_HD void put(char) { ++n; }
  TB_HD void copy(const char*, uint32_t len) { n += len; }
};

struct MetaWriteSink {
  char* p;
  uint32_t n = 0;
  TB_HD explicit MetaWriteSink(char* dst) : p(dst) {}
  TB_HD void put(char c) { p[n++] = c; }
  TB_HD void copy(const char* s, uint32_t len) {
    // eight loads, then eight stores: source and destination may alias for all the compiler
    // knows, and one load per store would wait out the memory latency once per byte
    char* d = p + n;
    uint32_t i = 0;
    for (; i + 8 <= len; i += 8) {
      const char c0 = s[i], c1 = s[i + 1], c2 = s[i + 2], c3 = s[i + 3];
      const char c4 = s[i + 4], c5 = s[i + 5], c6 = s[i + 6], c7 = s[i + 7];
      d[i] = c0; d[i + 1] = c1; d[i + 2] = c2; d[i + 3] = c3;
      d[i + 4] = c4; d[i + 5] = c5; d[i + 6] = c6; d[i + 7] = c7;
    }
    for (; i < len; ++i) d[i] = s[i];
    n += len;
  }
};

template <class Sink>
TB_HD_CALL void meta_u64(Sink& k, uint64_t v) {
  char buf[20];
  int n = 0;
  do {
    buf[n++] = (char)('0' + (int)(v % 10));
    v /= 10;
  } while (v);
  while (n) k.put(buf[--n]);
}

template <class Sink>
TB_HD void meta_i64(Sink& k, int64_t v) {
  if (v < 0) {
    k.put('-');
    meta_u64(k, (uint64_t)0 - (uint64_t)v);
  } else {
    meta_u64(k, (uint64_t)v);
  }
}

TB_HD uint64_t meta_f64_bits(double x) {
  union { double d; uint64_t u; } c;
  c.d = x;
  return c.u;
}

// format!("{:.prec}", x), prec 2 or 4 (rustfmt.h append_fixed's integer path): the exact binary
// value x = m * 2^-sh scaled by 10^prec and rounded half to even from the exact remainder.
// Returns false (nothing reproducible written) for a non-finite x or |x| >= 10^14.
template <class Sink>
TB_HD_CALL bool meta_fixed(Sink& k, double x, int prec) {
  const uint64_t bits = meta_f64_bits(x);
  const uint64_t frac = bits & 0xFFFFFFFFFFFFFull;
  const int be = (int)((bits >> 52) & 0x7FF);
  const bool neg = (bits >> 63) != 0;
  if (be == 0x7FF) return false;
  const double ax = neg ? -x : x;
  if (ax >= 1e14) return false;
  const uint64_t m = be ? (frac | (1ull << 52)) : frac;
  const int sh = be ? 1075 - be : 1074;  // |x| = m * 2^-sh; |x| < 10^14 < 2^47: sh >= 6
  const uint64_t p10 = prec == 2 ? 100ull : 10000ull;
  uint64_t qi = 0;
  if (m != 0 && sh < 120) {
    const unsigned __int128 scaled = (unsigned __int128)m * p10;
    unsigned __int128 q = scaled >> sh;
    const unsigned __int128 rem = scaled - (q << sh);
    const unsigned __int128 half = (unsigned __int128)1 << (sh - 1);
    if (rem > half || (rem == half && ((uint64_t)q & 1))) ++q;
    qi = (uint64_t)q;
  }
  if (neg) k.put('-');
  meta_u64(k, qi / p10);
  uint32_t fp = (uint32_t)(qi % p10);
  k.put('.');
  char fb[4];
  for (int i = prec - 1; i >= 0; --i, fp /= 10) fb[i] = (char)('0' + (int)(fp % 10));
  for (int i = 0; i < prec; ++i) k.put(fb[i]);
  return true;
}

// Rust f64 Display (rustfmt.h append_f64) for 0.125 <= x < 2: the shortest decimal that reads back
// as x, the closest to x among those, never an exponent. Exact interval search: with x = m * 2^-sh
// and S = sh + 2, a d-digit decimal D / 10^d round-trips iff lo * 10^d <= D * 2^S <= hi * 10^d for
// the halfway points lo / hi of x's neighbours (bounds included only for an even m, as the reader
// rounds half to even); 4m * 10^17 < 2^112. The language confidence is 1 / den, den in [1, 5].
// Returns false outside that range.
template <class Sink>
TB_HD_CALL bool meta_f64(Sink& k, double x) {
  if (!(x >= 0.125 && x < 2.0)) return false;
  const uint64_t bits = meta_f64_bits(x);
  const uint64_t m = (bits & 0xFFFFFFFFFFFFFull) | (1ull << 52);
  const int S = 1075 - (int)((bits >> 52) & 0x7FF) + 2;  // 54 .. 57
  const bool incl = (m & 1) == 0;
  // the gap below a power of two is half the gap above it
  const uint64_t lo = 4 * m - ((bits & 0xFFFFFFFFFFFFFull) == 0 ? 1 : 2), hi = 4 * m + 2, mid = 4 * m;
  const unsigned __int128 one = 1, mask = (one << S) - 1;
  unsigned __int128 p = 1;
  for (int d = 0; d <= 17; ++d, p *= 10) {
    const unsigned __int128 lo_n = lo * p, hi_n = hi * p;
    unsigned __int128 dmin = (lo_n + mask) >> S;
    if (!incl && (lo_n & mask) == 0) ++dmin;
    unsigned __int128 dmax = hi_n >> S;
    if (!incl && (hi_n & mask) == 0) {
      if (dmax == 0) continue;
      --dmax;
    }
    if (dmin > dmax) continue;
    // the candidate closest to x (no exact ties: x * 10^d is never a half integer for d <= 17)
    unsigned __int128 dc = (mid * p + (one << (S - 1))) >> S;
    if (dc < dmin) dc = dmin;
    if (dc > dmax) dc = dmax;
    const uint64_t D = (uint64_t)dc, P = (uint64_t)p;
    meta_u64(k, D / P);
    if (d > 0) {
      k.put('.');
      char fb[17];
      uint64_t f = D % P;
      for (int i = d - 1; i >= 0; --i, f /= 10) fb[i] = (char)('0' + (int)(f % 10));
      for (int i = 0; i < d; ++i) k.put(fb[i]);
    }
    return true;
  }
  return false;
}

// One output row. Appends '{' members '}' to the sink, or nothing for a row without members
// (a null row). `fail`: the row's first failing pipeline step (k_resolve), -1 for a kept row;
// tok[t]: the device token count of trailing TokenCounter t for a kept row. Returns false when
// the row holds a value the formatter does not reproduce (the batch is assembled on the host).
template <class Sink>
struct MetaRow {
  const DevMetaPlan& mp;
  const char* pool;  // the plan's literal pool, or a copy of it closer to the lanes (LDS)
  Sink& k;
  bool first = true, ok = true, any = false;

  TB_HD MetaRow(const DevMetaPlan& plan, const char* pool_, Sink& sink) : mp(plan), pool(pool_), k(sink) {}
  TB_HD void lit(MetaLit l) { k.copy(pool + l.off, l.len); }
  TB_HD void member() {  // separator in front of a member
    k.put(first ? '{' : ',');
    first = false;
  }
  TB_HD void reason_sep() {
    if (any) {
      k.put(';');
      k.put(' ');
    }
    any = true;
  }
  // multi-reason steps: the members' head on the first reason, "; " between reasons
  TB_HD void reason_begin(const DevMetaStep& ms, int r) {
    if (!any) {
      member();
      lit(ms.lit[ML_HEAD]);
    }
    reason_sep();
    lit(ms.lit[ML_REASON0 + 2 * r]);
  }
  TB_HD void reason_f2(const DevMetaStep& ms, int r, double v) {
    reason_begin(ms, r);
    ok &= meta_fixed(k, v, 2);
    lit(ms.lit[ML_REASON0 + 2 * r + 1]);
  }
  TB_HD void reason_i(const DevMetaStep& ms, int r, int64_t v) {
    reason_begin(ms, r);
    meta_i64(k, v);
    lit(ms.lit[ML_REASON0 + 2 * r + 1]);
  }
  TB_HD void reasons_end() {
    if (any) k.put('"');
    else ok = false;  // the resolve says this step failed, no branch of the chain agrees
  }

  TB_HD void passed(const DevGateStep& g, const DevMetaStep& ms, const int64_t* r) {
    if (g.kind == GK_LANGID) {
      langid(ms, r);
      return;
    }
    if (ms.lit[ML_PASSED].len) {
      member();
      lit(ms.lit[ML_PASSED]);
    }
  }

  TB_HD void langid(const DevMetaStep& ms, const int64_t* r) {
    const int64_t lang = r[0];
    if (lang < 0) return;
    if (lang >= kMetaLangs) {
      ok = false;
      return;
    }
    union { int64_t i; double d; } u;
    u.i = r[1];
    member();
    lit(ms.lit[ML_X0 + (int)lang]);
    ok &= meta_f64(k, u.d);
    k.put('"');
  }

  TB_HD void fineweb_fail(const DevMetaStep& ms, int r, double ratio) {
    member();
    lit(ms.lit[ML_REASON0 + 2 * r]);
    ok &= meta_fixed(k, ratio, 4);
    lit(ms.lit[ML_REASON0 + 2 * r + 1]);
  }

  TB_HD void failed(const DevGateStep& g, const DevMetaStep& ms, const int64_t* r) {
    any = false;
    switch (g.kind) {
      case GK_GOPHER_QUALITY: {
        const int64_t n = r[0];
        const double ncalc = (double)gate_max1(n);
        const double avg = n > 0 ? (double)r[1] / (double)n : 0.0;
        const double hash_ratio = (double)r[2] / ncalc;
        const double ell_ratio = (double)r[3] / ncalc;
        const double lcalc = (double)gate_max1(r[4]);
        const double bullet = (double)r[5] / lcalc;
        const double ell_lines = (double)r[6] / lcalc;
        const double alpha = (double)r[7] / ncalc;
        const uint32_t h = g.has;
        if ((h >> GQ_T_MIN_WORDS & 1) && n < g.i[0]) reason_i(ms, MQ_SHORT, n);
        if ((h >> GQ_T_MAX_WORDS & 1) && n > g.i[1]) reason_i(ms, MQ_LONG, n);
        if ((h >> GQ_T_MIN_AVG & 1) && avg < g.d[0]) {
          reason_begin(ms, MQ_BELOW_AVG);
          ok &= meta_fixed(k, avg, 2);
          lit(n == 0 ? ms.lit[ML_X0] : ms.lit[ML_REASON0 + 2 * MQ_BELOW_AVG + 1]);
        }
        if ((h >> GQ_T_MAX_AVG & 1) && n > 0 && avg > g.d[1]) reason_f2(ms, MQ_ABOVE_AVG, avg);
        if (h >> GQ_T_SYMBOL & 1) {
          if (hash_ratio > g.d[2]) reason_f2(ms, MQ_HASHES, hash_ratio);
          if (ell_ratio > g.d[2]) reason_f2(ms, MQ_ELLIPSIS, ell_ratio);
        }
        if ((h >> GQ_T_BULLET & 1) && bullet > g.d[3]) reason_f2(ms, MQ_BULLETS, bullet);
        if ((h >> GQ_T_ELL_LINES & 1) && ell_lines > g.d[4]) reason_f2(ms, MQ_ELL_LINES, ell_lines);
        if ((h >> GQ_T_ALPHA & 1) && alpha < g.d[5]) reason_f2(ms, MQ_ALPHA, alpha);
        if ((h >> GQ_T_MIN_STOP & 1) && g.i[2] > 0 && r[8] < g.i[2]) reason_i(ms, MQ_STOP, r[8]);
        reasons_end();
        return;
      }
      case GK_GOPHER_REP: {
        if (r[0] < 0) {
          member();
          lit(ms.lit[ML_X0]);
          return;
        }
        const double C = (double)gate_max1(r[0]);
        const double para_len = (double)gate_max1(r[1]);
        const double line_len = (double)gate_max1(r[4]);
        const uint32_t h = g.has;
        double v = (double)r[2] / para_len;
        if ((h >> GR_T_PARA & 1) && v > g.d[0]) reason_f2(ms, 0, v);
        v = (double)r[3] / C;
        if ((h >> GR_T_PARA_CHAR & 1) && v > g.d[1]) reason_f2(ms, 1, v);
        v = (double)r[5] / line_len;
        if ((h >> GR_T_LINE & 1) && v > g.d[2]) reason_f2(ms, 2, v);
        v = (double)r[6] / C;
        if ((h >> GR_T_LINE_CHAR & 1) && v > g.d[3]) reason_f2(ms, 3, v);
        int kk = 7;
        for (int t = 0; t < g.n_top; ++t, ++kk) {
          v = (double)r[kk] / C;
          if (g.top_n[t] > 0 && v > g.top_thr[t]) reason_f2(ms, 4 + t, v);
        }
        for (int t = 0; t < g.n_dup; ++t, ++kk) {
          v = (double)r[kk] / C;
          if (g.dup_n[t] > 0 && v > g.dup_thr[t]) reason_f2(ms, 4 + g.n_top + t, v);
        }
        reasons_end();
        return;
      }
      case GK_C4: {
        if (r[0] || r[1]) {
          member();
          lit(ms.lit[ML_HEAD]);
          if (r[0]) {
            reason_sep();
            lit(ms.lit[ML_X0]);
          }
          if (r[1]) {
            reason_sep();
            lit(ms.lit[ML_X1]);
          }
          k.put('"');
          return;
        }
        if (g.i[0] > 0 && r[5] < g.i[0]) {
          reason_i(ms, 0, r[5]);
          k.put('"');
          for (int j = 0; j < 3; ++j)
            if (r[2 + j]) {
              lit(ms.lit[MC_LINE0 + j]);
              meta_i64(k, r[2 + j]);
              k.put('"');
            }
          return;
        }
        ok = false;
        return;
      }
      case GK_FINEWEB: {
        const int64_t nl = r[0];
        if (nl == 0) {
          member();
          lit(ms.lit[ML_X0]);
          return;
        }
        double ratio = (double)r[1] / (double)nl;
        if (ratio < g.d[0] && !(ratio == 0.0 && g.flag)) return fineweb_fail(ms, 0, ratio);
        ratio = (double)r[2] / (double)nl;
        if (ratio > g.d[1]) return fineweb_fail(ms, 1, ratio);
        const int64_t tot = r[4];
        ratio = tot > 0 ? (double)r[3] / (double)tot : 0.0;
        if (ratio > g.d[2]) return fineweb_fail(ms, 2, ratio);
        const int64_t w = r[6], nls = r[5];
        if (w == 0) {
          if (nls > 0) {
            member();
            lit(ms.lit[ML_X1]);
          } else {
            ok = false;
          }
          return;
        }
        ratio = (double)nls / (double)w;
        if (ratio > g.d[3]) return fineweb_fail(ms, 3, ratio);
        ok = false;
        return;
      }
      case GK_LANGID:
        // the members do not depend on the outcome; the reason string is not metadata
        langid(ms, r);
        return;
      default:
        ok = false;
        return;
    }
  }
};

template <class Sink>
TB_HD bool meta_row(const DevResolve& rp, const DevMetaPlan& mp, const int64_t* const* recs, int64_t ndocs,
                    int64_t doc, int32_t fail, const int32_t* tok, Sink& k, const char* pool = nullptr) {
  MetaRow<Sink> row(mp, pool ? pool : mp.pool, k);
  bool reached = fail < 0;
  for (int s = 0; s < rp.gate.n_steps; ++s) {
    const DevGateStep& g = rp.gate.steps[s];
    const int64_t* r = recs[g.slot] + (int64_t)g.prefix * ndocs + doc * g.width;
    if (rp.step_index[s] == fail) {
      row.failed(g, mp.steps[s], r);
      reached = true;
      break;
    }
    row.passed(g, mp.steps[s], r);
  }
  if (!reached) row.ok = false;  // a failing step outside the plan
  if (fail < 0)
    for (int t = 0; t < mp.n_tokens; ++t) {
      if (tok[t] < 0) {
        row.ok = false;  // -2: counted by the host tokenizer, -1: tokenizer error
        continue;
      }
      row.member();
      row.lit(mp.token);
      meta_i64(k, tok[t]);
      k.put('"');
    }
  if (!row.first) k.put('}');
  return row.ok;
}

}  // namespace tb
