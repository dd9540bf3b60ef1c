"""dec_ngram_kernel alone, through fw_test_ngram_rows, against the float64 restatement of tests/ngram_refs.py within the
bound of the contract's float32 roundings; untouched ids, -inf logits and skipped rows bit for bit.  Both row forms
(0 = decode step: one history length per launch, two beams per chunk, a done chunk; 1 = scoring: ragged histories, rows
without a target).  Four consecutive vocabulary sizes put a row start at every 16-byte residue."""
import numpy as np
import pytest

import ngram_refs as nr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config("micro")
    model = Whisper("synthetic:ngram", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=5)},
                    max_batch_size=2, max_beam_size=5)
    yield model._replicas[0].handle
    del model


@pytest.mark.parametrize("N", [1, 2, 3, 5])
@pytest.mark.parametrize("V", [1021, 1022, 1023, 1024])
def test_kernel_against_the_reference(handle, V, N):
    eot, tsb = V - 120, V - 80
    m, hists = nr.model_of_order(N, V, eot, tsb)
    lm = nr.Model(m)
    # scoring form: every history in one launch, rows 2 and 7 without a target
    logits = nr.logits_of(len(hists), V)
    got = nr.rows_gpu(handle, logits, hists, lm, eot, tsb, form=1, done=[int(r in (2, 7)) for r in range(len(hists))])
    nr.check(got, logits, *nr.fused_rows(logits, m, hists, eot, tsb, skipped=(2, 7)))
    # decode-step form: the histories of one length, twice over as the two beams of a chunk each, the last chunk done
    for n in sorted({len(h) for h in hists}):
        rows = [h for h in hists if len(h) == n for _ in range(2)] + [[0] * n] * 2
        logits = nr.logits_of(len(rows), V, seed=n)
        done = [0] * (len(rows) // 2 - 1) + [1]
        got = nr.rows_gpu(handle, logits, rows, lm, eot, tsb, form=0, K=2, done=done)
        nr.check(got, logits, *nr.fused_rows(logits, m, rows, eot, tsb, skipped=(len(rows) - 2, len(rows) - 1)))
