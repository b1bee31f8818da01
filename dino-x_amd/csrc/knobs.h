// knobs.h -- every DINOX_* environment switch the library reads, and the only getenv in csrc/ (tests/test_knobs_cpu.py holds both).
// All of them are A/B and test switches: unset, every rule is the measured policy written next to the launch it steers.  The table
// is an index; why a rule exists stays beside the rule.
//
// Lifetime: "call" = read at every launch, so one process (a tool, a test with monkeypatch.setenv) can flip it between launches;
//           "once" = read at the first launch that reaches it and held in a function-local static at the place of use.
//
//   knob                    values (default)                                                              used in                  read
//   DINOX_NT_PP             ping-pong kernels: 0 never, 1 by shape only, 2 / 3 force 256 x 128 / 256 x 256   gemm_bf16.hip            call
//                           tiles (unset: measured policy, nt_pp_choice)
//   DINOX_NT_PP384          0 never, 1 every product in the full-row kernel's envelope (unset: measured)    gemm_bf16.hip            call
//   DINOX_FC1_AREG          non-zero: GELU epilogue at K < 768 back on the register-prefetch kernel (off)    gemm_bf16.hip            call
//   DINOX_NT_AREG_MAXK      longest K that takes the register-prefetch form (576)                           gemm_bf16.hip            call
//   DINOX_NT_NO_AREG        set: register-prefetch form off (unset)                                         gemm_bf16.hip            once
//   DINOX_NT_STORES         register-prefetch kernel's output stores: 0 plain, 1 non-temporal, 2 / 3 only    gemm_bf16_areg.hip       call
//                           outputs of >= 10 / < 10 column tiles (unset: non-temporal for bf16 outputs)
//   DINOX_NT_BK             32 | 64: K-step depth of the LDS-DMA NT kernel (0 = by shape)                    gemm_bf16_glds.hip       once
//   DINOX_NT_BM             128 | 256: its tile height (128)                                                gemm_bf16_glds.hip       once
//   DINOX_PP_ORDER          ping-pong kernels' tile order: 0 contiguous, 1 XCD interleave, +256 (1)          kernels.h (pp, pp128)    call
//   DINOX_PP_STAGGER        their workgroup start stagger in cycles, 0 = off (unset: by epilogue and K)      kernels.h (pp, pp128)    call
//   DINOX_ROWLN_PP          product + LayerNorm on the full-row kernel: 0 never, 1 whole envelope            gemm_bf16_rowln.hip      call
//                           (unset: bf16 y and M >= 40000)
//   DINOX_ROWLN             block plan, product + LayerNorm as one launch: 0 never, 1 proj and fc2           block.hip                call
//                           (unset: proj; fc2 where DINOX_ROWLN_PP's kernel takes it)
//   DINOX_ROWLN_FC2         0: fc2 + LayerNorm stays two launches on the full-row kernel's shapes too (unset) block.hip                call
//   DINOX_LNBWD_PP          block plan, dX product + LayerNorm backward as one launch: 0 never, 1 whole      block.hip                call
//                           envelope (unset: M >= 8192)
//   DINOX_QKV_FUSED         block plan, no-grad qkv projection + attention as one launch: 0 never, 1 every   block.hip                call
//                           width (unset: D <= 512); attention_bf16.hip's notes name it
//   DINOX_TN_BIG_OFF        set: dW products stay on 128 x 128 tiles (unset)                                gemm_bf16_tnbig.hip      once
//   DINOX_TN_FORM           1 | 2 | 3 force a big-tile shape (0 = cheapest plan)                            gemm_bf16_tnbig.hip      call
//   DINOX_TN_PP             dW K loop: 0 waves in step, 1 anti-phase 32x32x16, 2 anti-phase 16x16x32 (2)     gemm_bf16_tnbig.hip      call
//   DINOX_LN_NO384          set: generic LayerNorm kernels at width 384 (unset)                             layernorm.hip            once
//   DINOX_ATTN_NO_FLASH     set: shapes outside the whole-strip kernels skip attention_flash.hip (unset)     attention.hip            call
//   DINOX_ATTN_NO_PERSIST   set: non-persistent attention forward (unset)                                   attention_bf16.hip       once
//   DINOX_ATTN_BWD_SPLIT    set: two-kernel attention backward (unset)                                      attention_bf16.hip       once
//
// Named in csrc/ but not read here:
//   DINOX_PLAIN_OUT_STORES  compile-time macro (common.h, store_stream): ordinary instead of non-temporal stores, alternate builds only
#pragma once
#include <cstdlib>

namespace dinox {

static inline bool knob_set(const char* name) { return getenv(name) != nullptr; }
static inline int knob_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

}  // namespace dinox
