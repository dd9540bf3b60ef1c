"""What truncated sampling costs per decode step: time per launch of the PF_DEC_SAMPLE family (`dec_sample`: the rules
kernel, the beam update and the step advance of one step, HIP-event timing through fw_prof_*) in sampling runs of 40 rows
(8 chunks x 5 hypotheses, 40 steps, <eot> suppressed) at the large-v3 vocabulary on the micro geometry: plain, and
truncating with (top_k, top_p) = (5, 1), (0, 0.9), (50, 0.9).  Steps are launched eagerly (FWAMD_NO_GRAPH=1).
usage: python profiles/sampling_trunc_cost.py LABEL [plain-only]
       FWAMD_LIB=/path/to/another/libfwamd.so python profiles/sampling_trunc_cost.py parent plain-only
One JSON line per repetition on stdout, then the best of five per configuration."""
import json
import os
import sys

os.environ["FWAMD_NO_GRAPH"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from conftest import bench_audio  # noqa: E402
import sampling_trunc_refs as st  # noqa: E402
from faster_whisper_amd import Whisper, synthetic_weights  # noqa: E402

label = sys.argv[1]
plain_only = len(sys.argv) > 2
cfg = st.vocab_cfg("large-v3")
w = synthetic_weights(cfg, seed=7, peaked=True)
model = Whisper("synthetic:m", device="cuda", files={"config": cfg, "weights": w}, max_batch_size=8, max_beam_size=5)
model.set_decode_lanes(1)
batch = [bench_audio(480000, seed=60 + i) for i in range(8)]
enc = model.encode_pcm(batch)
prompt = list(cfg.sot_sequence) + [cfg.no_timestamps]
NH, STEPS = 5, 40
base = dict(beam_size=1, num_hypotheses=NH, sampling_topk=0, sampling_temperature=1.0, seed=3, max_length=len(prompt) + STEPS,
            suppress_tokens=[cfg.sot, cfg.no_speech, cfg.eot])
configs = [("plain", {})] + ([] if plain_only else [("k5", dict(top_k=5)), ("p0.9", dict(top_p=0.9)), ("k50 p0.9", dict(top_k=50, top_p=0.9))])
for name, kw in configs:
    model.generate(enc, [prompt] * 8, **base, **kw)            # warm-up
    best = None
    for rep in range(5):
        model.profile(True)
        model.generate(enc, [prompt] * 8, **base, **kw)
        r = model.profile_report()
        model.profile(False)
        fam = {k: v for k, v in r.items() if "sample" in k.lower()}
        (key, v), = fam.items()
        us = 1000.0 * v["ms"] / max(1, v["launches"])
        best = us if best is None else min(best, us)
        rec = dict(label=label, config=name, rows=8 * NH, family=key, launches=v["launches"], us_per_launch=round(us, 2), rep=rep)
        print(json.dumps(rec), flush=True)
    print(f"{label} {name}: rows {8 * NH}, best of 5: {best:.2f} us per launch of {key}")
