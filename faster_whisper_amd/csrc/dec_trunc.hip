// The TRUNC instantiations of the logits-rules kernel (truncated sampling, fw_generate_trunc): the kernel template, its TRUNC
// stage (lp_trunc_cut) and the row helpers are dec_vocab.hip's, included here as text; this unit instantiates
// dec_logits_process_kernel<true, TXI, ALT, true> and nothing else, so that dec_vocab.hip compiles to the kernels it always
// compiled to.
#define DEC_VOCAB_TRUNC_UNIT
#include "dec_vocab.hip"

namespace fwd {

void launch_logits_process_trunc(hipStream_t st, const GenDev& gp, float* logits, const unsigned long long* sup_bits,
                                 const int* hist2, const float* cum2, const int* d_step, const int* done, float* cand_val,
                                 int* cand_tok, float* cand_lp, const SmpRow* smp_tab, int* alt_tok, float* alt_lp,
                                 const TruncRow* trunc_tab) {
  if (!gp.sample || !smp_tab || !trunc_tab) return;   // (launch_logits_process has checked: nothing is launched)
  const bool wide = gp.ts_begin >= 48 * LP_THREADS;   // as launch_logits_process
  const bool alt = gp.n_alt > 0 && alt_tok && alt_lp;
#define LP_GO(TXI, ALT) \
  dec_logits_process_kernel<true, TXI, ALT, true><<<gp.R, LP_THREADS, 0, st>>>(gp, logits, sup_bits, hist2, cum2, d_step, done, cand_val, cand_tok, cand_lp, smp_tab, alt_tok, alt_lp, trunc_tab)
  if (alt) { if (wide) LP_GO(48, true); else LP_GO(0, true); }
  else { if (wide) LP_GO(48, false); else LP_GO(0, false); }
#undef LP_GO
}

}  // namespace fwd
