#pragma once
#include "doc_ctx.h"
#include "langid.h"

namespace tb {

// Language-id record straight from the UTF-8 bytes: every code point position (a UTF-8 lead
// byte, as decode() defines them) of the first kLidMaxCps code points, plus the virtual end
// position, emits the 1..4-grams ending there (lid_grams_at); their int8 embedding rows are summed
// exactly. Neighbouring letters are found by stepping back to the previous lead bytes, so no
// per-code-point arrays are needed. The device runs its own kernel for this (k_langid_mfma,
// same sums); this version runs inside the stage emulation on the host.
template <class P, int D>
TB_HD void langid_sums(DocCtx<P>& x, const uint8_t* b, uint32_t n, const LidTables& lt, int64_t* sums) {
  const UcdView ucd = x.ucd;
  const auto mark = x.mark();
  int32_t* tmp = x.template alloc_hot<int32_t>(64 * D);
  uint32_t* limb = x.template alloc_hot<uint32_t>(1);
  if (x.overflow) return;
  // byte offset of code point kLidMaxCps (the cut), or n
  x.par.single([&]() { *limb = n; });
  x.par.sync();
  if (n > (uint32_t)kLidMaxCps) {
    x.par.template compact<int>(
        n, [&](uint32_t i, int&) { return utf8_is_lead(b[i]); },
        [&](uint32_t i, uint32_t k, int&) { if (k == (uint32_t)kLidMaxCps) *limb = i; });
    x.par.sync();
  }
  const uint32_t lim = *limb;
  // A lane visits ceil((lim + 1) / 64) <= 257 byte positions (lim <= 4 * kLidMaxCps) with at most
  // 4 grams each and |row value| <= 2^15: int32 partials cannot overflow.
  x.par.template accum_rows<D>(
      lim + 1,
      [&](uint32_t s, int32_t* part) {
        if (s < lim && !utf8_is_lead(b[s])) return;
        const uint32_t l0 = s < lim ? lid_letter(ucd, b, n, s) : 0u;
        const int64_t p1 = prev_lead(b, s);
        const int64_t p2 = p1 >= 0 ? prev_lead(b, p1) : -1;
        const int64_t p3 = p2 >= 0 ? prev_lead(b, p2) : -1;
        part[D - 1] += lid_grams_n(lid_letter(ucd, b, n, p3), lid_letter(ucd, b, n, p2),
                                   lid_letter(ucd, b, n, p1), l0, [&](uint32_t g, int order) {
                                     lid_add_emb(lt.E, g, order, part);
                                   });
      },
      tmp, sums);
  x.reset(mark);
}

// The record from those sums: lid_record_v3, the same integers as the device's MFMA tile.
template <class P>
TB_HD void langid_record(DocCtx<P>& x, const uint8_t* b, uint32_t n, const LidTables& lt, int64_t* r) {
  const auto mark = x.mark();
  int64_t* sums = x.template alloc_hot<int64_t>(kLidDim + 1);  // shared by the lanes
  if (x.overflow) return;
  langid_sums<P, kLidDim + 1>(x, b, n, lt, sums);
  if (x.overflow) return;
  x.par.single([&]() { lid_record_v3(sums, sums[kLidDim], lt, r); });
  x.par.sync();
  x.reset(mark);
}

}  // namespace tb
