// Per-document analysis algorithms shared by the HIP kernels and the host emulation, one header per
// family: a kernel unit includes the families it calls, csrc/host/devplan_build.cpp this umbrella.
//   doc_ctx.h        DocCtx and its arenas, phase ids, DOC_* flags, Cps, PHView, PreDoc, Words, Lines
//   doc_text.h       decode, prefix_hash8, words, rust_lines, SWAR helpers;  doc_dedup.h: canonicalize, dup_spans
//   gopher_rep.h     gopher_rep_record, GrExport, dup_walk[_wave], gr_top / gr_dup_one_order
//   c4_pass_a.h      c4_pass_a and its paths, c4_byte_scan, count_sentences_upto
//   stage_analyze.h  analyze_stage, StageOut, is_stop_word, gq_byte_counts;  doc_langid.h: langid_record (emulation)
#pragma once
#include "c4_pass_a.h"
#include "doc_ctx.h"
#include "doc_dedup.h"
#include "doc_langid.h"
#include "doc_text.h"
#include "gopher_rep.h"
#include "stage_analyze.h"
