"""Weight naming + the deterministic synthetic weight generator.

No Whisper checkpoint exists in the build environment, so parity
tests and the benchmark use seeded random weights of the exact architecture.  The same
dict (name -> numpy array) feeds the HIP engine (via fw_model_create) and the CPU oracle.

Tensor names / shapes (PyTorch [out, in] convention, biases 1-D):
  enc.conv1.w [d, n_mels, 3]  enc.conv1.b [d]   enc.conv2.w [d, d, 3]  enc.conv2.b [d]
  enc.pos [1500, d]
  enc.{i}.ln1.g/b  enc.{i}.attn.qkv.w [3d, d] (q rows, k rows, v rows)  enc.{i}.attn.qkv.b [3d] (k part = 0)
  enc.{i}.attn.out.w [d, d] / .b   enc.{i}.ln2.g/b   enc.{i}.ffn1.w [4d, d] / .b   enc.{i}.ffn2.w [d, 4d] / .b
  enc.ln_post.g/b
  dec.tok_emb [V, d]  dec.pos [448, d]
  dec.{i}.ln1.g/b  dec.{i}.self.qkv.w/.b  dec.{i}.self.out.w/.b
  dec.{i}.ln2.g/b  dec.{i}.cross.q.w/.b  dec.{i}.cross.kv.w [2d, d] (k rows, v rows) / .b (k part = 0)
  dec.{i}.cross.out.w/.b  dec.{i}.ln3.g/b  dec.{i}.ffn1.w/.b  dec.{i}.ffn2.w/.b
  dec.ln.g/b
"""
import os
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import Dict

import numpy as np

from .config import WhisperConfig


def weight_shapes(cfg: WhisperConfig) -> Dict[str, tuple]:
    d = cfg.d_model
    s = {
        "enc.conv1.w": (d, cfg.n_mels, 3), "enc.conv1.b": (d,),
        "enc.conv2.w": (d, d, 3), "enc.conv2.b": (d,),
        "enc.pos": (cfg.n_audio_ctx, d),
    }
    for i in range(cfg.n_enc_layers):
        p = f"enc.{i}."
        s.update({p + "ln1.g": (d,), p + "ln1.b": (d,), p + "attn.qkv.w": (3 * d, d), p + "attn.qkv.b": (3 * d,),
                  p + "attn.out.w": (d, d), p + "attn.out.b": (d,), p + "ln2.g": (d,), p + "ln2.b": (d,),
                  p + "ffn1.w": (4 * d, d), p + "ffn1.b": (4 * d,), p + "ffn2.w": (d, 4 * d), p + "ffn2.b": (d,)})
    s.update({"enc.ln_post.g": (d,), "enc.ln_post.b": (d,),
              "dec.tok_emb": (cfg.n_vocab, d), "dec.pos": (cfg.n_text_ctx, d)})
    for i in range(cfg.n_dec_layers):
        p = f"dec.{i}."
        s.update({p + "ln1.g": (d,), p + "ln1.b": (d,), p + "self.qkv.w": (3 * d, d), p + "self.qkv.b": (3 * d,),
                  p + "self.out.w": (d, d), p + "self.out.b": (d,), p + "ln2.g": (d,), p + "ln2.b": (d,),
                  p + "cross.q.w": (d, d), p + "cross.q.b": (d,), p + "cross.kv.w": (2 * d, d),
                  p + "cross.kv.b": (2 * d,), p + "cross.out.w": (d, d), p + "cross.out.b": (d,),
                  p + "ln3.g": (d,), p + "ln3.b": (d,), p + "ffn1.w": (4 * d, d), p + "ffn1.b": (4 * d,),
                  p + "ffn2.w": (d, 4 * d), p + "ffn2.b": (d,)})
    s.update({"dec.ln.g": (d,), "dec.ln.b": (d,)})
    return s


def sinusoids(length: int, channels: int) -> np.ndarray:
    """Whisper's fixed encoder positions: [sin | cos] concatenated."""
    inc = np.log(10000.0) / (channels // 2 - 1)
    inv = np.exp(-inc * np.arange(channels // 2))
    t = np.arange(length)[:, None] * inv[None, :]
    return np.concatenate([np.sin(t), np.cos(t)], axis=1).astype(np.float32)


PEAK_ALPHA = 24.0   # weight of the two candidate embeddings in a peaked position embedding (synthetic_weights)


def synthetic_weights(cfg: WhisperConfig, seed: int = 1234, dtype=np.float16, peaked: bool = False
                      ) -> Dict[str, np.ndarray]:
    """Seeded random weights, scaled so activations stay O(1) through 32 layers in fp16.
    Each tensor has its own stream (seed, crc32(name)), so the values do not depend on
    generation order.  Values are rounded to `dtype` (fp16 by default = what the engine stores).

    peaked=True ("hard parts"): random weights give logits whose top-1 / top-2 margin is of the
    size of fp16 evaluation noise at some step of every transcript, so literal greedy-id equality between the fp16
    engine and the fp32 oracle cannot be asserted on them.  A trained model is PEAKED: one or two tokens carry the
    probability mass.  The peaked variant gets there by construction: the learned position embedding of decoder
    position p additionally carries PEAK_ALPHA x (E[a_p] + beta_p E[b_p]), beta_p in [0.55, 0.8], for two pseudo-random
    text tokens a_p, b_p of the tied embedding E, so that after the final LayerNorm the logits of a_p and b_p stand far
    above the other 51 864 and a_p leads b_p by a margin of several units, not 1e-2 (with beta = 1 the two tie at the
    noise level whenever |E[a]| ~ |E[b]|: measured 2 of 64 steps on large-v3).  The transcript is then a_P-1, a_P, ...:
    it differs from step to step; the audio moves the margins, not the winner (random weights attend nearly uniformly
    over the 1 500 frames, so the cross-attention output hardly depends on the audio — measured)."""
    d = cfg.d_model

    def make(item):
        name, shape = item
        rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
        if name == "enc.pos":
            w = sinusoids(cfg.n_audio_ctx, d)
        elif name.endswith(".g"):
            w = 1.0 + 0.1 * rng.standard_normal(shape, dtype=np.float32)
        elif name.endswith("ln1.b") or name.endswith("ln2.b") or name.endswith("ln3.b") or name.endswith("ln.b") \
                or name.endswith("ln_post.b"):
            w = 0.05 * rng.standard_normal(shape, dtype=np.float32)
        elif name.endswith(".b"):
            w = 0.02 * rng.standard_normal(shape, dtype=np.float32)
            if name.endswith("qkv.b"):
                w[d:2 * d] = 0.0   # Whisper's key projection has no bias
            if name.endswith("cross.kv.b"):
                w[:d] = 0.0
        elif name == "dec.tok_emb":
            # tied input/output embedding: keep it small next to the positions, otherwise the
            # "repeat the input token" attractor makes every synthetic transcript constant
            w = 0.1 * rng.standard_normal(shape, dtype=np.float32)
        elif name == "dec.pos":
            w = 0.6 * rng.standard_normal(shape, dtype=np.float32)
        elif name.startswith("enc.conv"):
            fan_in = shape[1] * shape[2]
            w = (1.0 / np.sqrt(fan_in)) * rng.standard_normal(shape, dtype=np.float32)
        else:  # linear [out, in]
            scale = 0.8 / np.sqrt(shape[1])
            if name.endswith("ffn2.w") or name.endswith("out.w"):
                scale *= 0.5  # residual branches: keep the stream from growing
            w = rng.standard_normal(shape, dtype=np.float32)
            w *= scale
        return name, np.ascontiguousarray(w.astype(dtype))

    # the streams are independent and numpy fills arrays without the GIL: large-v3's 1.5 G values take seconds on a
    # thread pool instead of most of the benchmark's start-up on one core; the result does not depend on the pool
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        out = dict(pool.map(make, weight_shapes(cfg).items()))
    return make_peaked(cfg, out, seed) if peaked else out


def make_peaked(cfg: WhisperConfig, weights: Dict[str, np.ndarray], seed: int = 1234) -> Dict[str, np.ndarray]:
    """the peaked variant of a weight set (see synthetic_weights): only `dec.pos` differs, every other tensor is shared"""
    ids = peaked_candidates(cfg, seed)
    emb = weights["dec.tok_emb"].astype(np.float32)
    beta = np.random.default_rng([seed, zlib.crc32(b"peaked.beta")]).uniform(0.55, 0.8, size=len(ids)).astype(np.float32)
    pos = weights["dec.pos"].astype(np.float32) + PEAK_ALPHA * (emb[ids[:, 0]] + beta[:, None] * emb[ids[:, 1]])
    out = dict(weights)
    out["dec.pos"] = np.ascontiguousarray(pos.astype(weights["dec.pos"].dtype))
    return out


def peaked_candidates(cfg: WhisperConfig, seed: int = 1234) -> np.ndarray:
    """[n_text_ctx][2]: the two candidate tokens (distinct) of every decoder position of synthetic_weights(peaked=True):
    plain text ids — no special token, nothing a test suppresses"""
    rng = np.random.default_rng([seed, zlib.crc32(b"peaked.pairs")])
    lo, hi = (1000, min(cfg.eot, 50000)) if cfg.eot > 2000 else (10, cfg.eot)   # (the micro test vocabulary)
    a = rng.integers(lo, hi, size=cfg.n_text_ctx)
    b = lo + (a - lo + 1 + rng.integers(0, hi - lo - 1, size=cfg.n_text_ctx)) % (hi - lo)
    return np.stack([a, b], axis=1)
