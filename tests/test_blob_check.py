"""The packed weight blob, without a GPU: its bytes are pinned (tests/golden/blob_sha256.json, recorded from the build
before the packer and the binder became two visitors of one weight list), and the host-side check that model creation
makes of a blob before it binds it (fw_test_blob_check) passes what the packer writes and refuses, by tensor name, a blob
whose entries do not say what the config implies."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from faster_whisper_amd import _lib, get_config, synthetic_weights
from faster_whisper_amd.backend import pack_blob
from test_oracle_int8 import _Entry, _Hdr

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "blob_sha256.json")))
TYPES = {"float16": _lib.COMPUTE_FLOAT16, "int8_float16": _lib.COMPUTE_INT8_FLOAT16}


@pytest.fixture(scope="module")
def weights():
    return {name: (get_config(name), synthetic_weights(get_config(name), seed=4)) for name in ("micro", "tiny.en")}


def _pack(weights, monkeypatch, size, ctype, plain):
    monkeypatch.delenv("FWAMD_LN_UNFOLD", raising=False)
    monkeypatch.delenv("FWAMD_PACK_PLAIN", raising=False)
    if plain:
        monkeypatch.setenv("FWAMD_PACK_PLAIN", "1")
    cfg, w = weights[size]
    return pack_blob(cfg, w, TYPES[ctype])


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_blob_bytes_are_pinned(weights, monkeypatch, case):
    size, ctype, plain = case.split("/")
    blob = _pack(weights, monkeypatch, size, ctype, plain == "plain")
    assert blob.size == GOLDEN[case]["bytes"]
    assert hashlib.sha256(blob.tobytes()).hexdigest() == GOLDEN[case]["sha256"]


def test_plain_forms_do_not_travel_in_int8():
    for size in ("micro", "tiny.en"):
        assert GOLDEN[f"{size}/int8_float16/plain"] == GOLDEN[f"{size}/int8_float16/default"]


def _check(blob):
    lib = _lib.load()
    rc = lib.fw_test_blob_check(_lib.ptr(blob), blob.size)
    return rc, lib.fw_last_error().decode()


def _entries(blob):
    """name -> (byte position of the entry in the blob, the entry)"""
    h = _Hdr.from_buffer_copy(blob[:C.sizeof(_Hdr)].tobytes())
    out = {}
    for i in range(h.n_tensors):
        pos = C.sizeof(_Hdr) + i * C.sizeof(_Entry)
        e = _Entry.from_buffer_copy(blob[pos:pos + C.sizeof(_Entry)].tobytes())
        out[e.name.decode()] = (pos, e)
    return h, out


def _edited(blob, name, edit):
    """a copy of blob with edit(entry) applied to the entry `name` ("" = the last entry); returns (copy, entry name)"""
    out = blob.copy()
    h, ents = _entries(out)
    if not name:
        name = max(ents, key=lambda n: ents[n][0])
    pos, e = ents[name]
    edit(e, h)
    out[pos:pos + C.sizeof(_Entry)] = np.frombuffer(bytes(e), dtype=np.uint8)
    return out, name


@pytest.fixture(scope="module")
def micro_blobs(weights):
    mp = pytest.MonkeyPatch()
    try:
        return {(ctype, plain): _pack(weights, mp, "micro", ctype, plain)
                for ctype, plain in (("float16", False), ("float16", True), ("int8_float16", False))}
    finally:
        mp.undo()


@pytest.mark.parametrize("ctype,plain", [("float16", False), ("float16", True), ("int8_float16", False)])
def test_blob_check_passes_what_the_packer_writes(micro_blobs, ctype, plain):
    rc, err = _check(micro_blobs[(ctype, plain)])
    assert rc == _lib.FW_OK, err


def _halve_k(e, h):
    e.dims[1] //= 2


def _unpadded_vocab(e, h):
    assert e.dims[0] == (h.cfg.n_vocab + 15) // 16 * 16 != h.cfg.n_vocab   # (micro's vocabulary is no whole tile)
    e.dims[0] = h.cfg.n_vocab


def _dtype_int8(e, h):
    e.dtype = 2


def _past_the_end(e, h):
    e.offset = (h.total_bytes - e.nbytes) // 256 * 256 + 256
    assert e.offset + e.nbytes > h.total_bytes


def _rename(e, h):
    e.name = b"enc.1.ln2.x"


@pytest.mark.parametrize("name,edit", [
    ("dec.0.self.qkv.wf", _halve_k),
    ("dec.logits.wf", _unpadded_vocab),
    ("enc.0.ffn1.w", _dtype_int8),
    ("", _past_the_end),
    ("enc.1.ln2.g", _rename),
], ids=["dims1_halved", "vocab_unpadded", "dtype", "offset_past_end", "missing"])
def test_blob_check_refuses_a_wrong_entry(micro_blobs, name, edit):
    bad, name = _edited(micro_blobs[("float16", False)], name, edit)
    rc, err = _check(bad)
    assert rc == _lib.FW_EINVAL and f"'{name}'" in err, (rc, err)


def test_blob_check_refuses_another_compute_type(micro_blobs):
    bad = micro_blobs[("float16", False)].copy()
    h = _Hdr.from_buffer_copy(bad[:C.sizeof(_Hdr)].tobytes())
    h.compute_type = _lib.COMPUTE_INT8_FLOAT16
    bad[:C.sizeof(_Hdr)] = np.frombuffer(bytes(h), dtype=np.uint8)
    rc, err = _check(bad)
    # the first tensor the int8 weight list has and the fp16 blob lacks
    assert rc == _lib.FW_EINVAL and "'enc.0.attn.qkv.wq'" in err, (rc, err)
