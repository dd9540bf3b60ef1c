"""The workload behind the kernel-trace comparison of dec_automaton_kernel with dec_constrain_kernel ("Automaton-
constrained decoding"): constrain_cost.py's setting — large-v3 geometry, synthetic weights, bench.py's audio, prompt and
suppress list, beam 5, the constraint's full list of 128 phrases x 32 tokens, a budget of 32 new tokens, so every call
decodes exactly 32 steps with text histories of 0 .. 31 ids — decoded `--calls` times after two warm-up calls, with

  --kind constraint   generate(constraint=list): dec_constrain_kernel (FWAMD_LIB=<the parent commit's libfwamd.so> for the
                      parent's kernel), or
  --kind automaton    generate(automaton=Whisper.automaton(Grammar.phrases(list))): dec_automaton_kernel, the same language.

Run under a kernel trace, steps launched eagerly:
    FWAMD_NO_GRAPH=1 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/automaton_trace.py --kind K --batch B
(--batch 16: 80 logits rows; --batch 128: 640, a full lane); the per-kernel average of the *_kernel_stats.csv it leaves is the
figure quoted.

usage: python profiles/automaton_trace.py --kind constraint|automaton [--batch 16] [--calls 8] [--model large-v3]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STEPS = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("constraint", "automaton"), required=True)
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=8)
    args = ap.parse_args()
    import bench
    from faster_whisper_amd import get_config
    from faster_whisper_amd.grammar import Grammar
    cfg = get_config(args.model)
    bargs = argparse.Namespace(model=args.model, batch=args.batch, beam=5, workers=1, compute_type="float16",
                               merge_fill=None, merge_wait_ms=None)
    model, _ = bench.build_backend(bargs, cfg, 0, 1, 0)
    enc = model.encode_pcm(bench.synth_chunks(args.batch, 1000))
    prompt = list(cfg.sot_sequence) + [cfg.no_timestamps]
    sup = [cfg.sot, cfg.sot_prev, cfg.sot_lm, cfg.no_speech, cfg.translate, cfg.transcribe]
    rng = np.random.default_rng(0)
    text = np.setdiff1d(np.arange(1000, 40000), np.asarray(sup + list(cfg.suppress_begin)))
    phrases = [[int(t) for t in rng.choice(text, size=STEPS)] for _ in range(128)]
    extra = (dict(constraint=model.constraint_list(phrases)) if args.kind == "constraint"
             else dict(automaton=model.automaton(Grammar.phrases(phrases))))
    for _ in range(2 + args.calls):
        res = model.generate(enc, [prompt] * args.batch, beam_size=5, patience=1.0, length_penalty=1.0,
                             max_length=len(prompt) + STEPS, return_scores=True, return_no_speech_prob=True,
                             suppress_blank=True, suppress_tokens=sup, **extra)
        assert all(len(r.sequences_ids[0]) == STEPS for r in res)
    model.synchronize()
    print(f"{args.kind}: {2 + args.calls} calls x {STEPS} steps, {args.batch} chunks x beam 5")


if __name__ == "__main__":
    main()
