"""The device sampler's host side (no GPU): exports, argument validation, parameter ranges, the counter-based uniform, and the float64
restatement that tests/test_gpu_sample.py holds the kernel to -- pinned here to HF's logits processors, which is what the reference's
``generate`` call runs (inference/base.py:10-16, transformers/generator.py:50-58)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import sample_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import paroquant_amd  # noqa: F401
    from paroquant_amd import _native
    return _native.load()


def test_sampler_exports_and_abi_version(lib):
    from paroquant_amd import _native
    hdr = open(os.path.join(ROOT, "include", "paro_abi.h")).read()
    for name in ("paro_sample_workspace_bytes", "paro_sample_uniform", "paro_sample_advance"):
        assert name in _native.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert "paro_sample_params_t" in hdr
    assert ctypes.sizeof(_native.ParoSampleParams) == 24
    assert _native.ParoSampleParams.seed.offset == 16 and _native.ParoSampleParams.top_k.offset == 12
    assert lib.paro_abi_version() == _native.PARO_ABI_VERSION == 20       # purely additive exports


def test_sample_advance_validation_without_gpu(lib):
    one = ctypes.c_void_p(1)
    V = 1000
    n = lib.paro_sample_workspace_bytes(V)
    assert n >= 16 + 4 * V + V
    assert lib.paro_sample_workspace_bytes(0) == -1 and lib.paro_sample_workspace_bytes(2 ** 31) == -1
    assert lib.paro_sample_workspace_bytes(2 ** 31 - 1) > 5 * (2 ** 31 - 1)
    good = dict(logits=one, vocab=V, dt=1, params=one, token=one, pos=one, out=one, out_len=8, advance=1, ws=one, ws_bytes=n)

    def call(**kw):
        a = {**good, **kw}
        return lib.paro_sample_advance(a["logits"], a["vocab"], a["dt"], a["params"], a["token"], a["pos"], a["out"], a["out_len"],
                                       a["advance"], a["ws"], a["ws_bytes"], None)

    for key in ("logits", "params", "token", "pos", "ws"):
        assert call(**{key: None}) == -1, key
        assert b"null" in lib.paro_last_error()
    assert call(vocab=0) == -1 and b"vocab" in lib.paro_last_error()
    assert call(vocab=-3) == -1 and b"vocab" in lib.paro_last_error()
    for dt in (0, 3):
        assert call(dt=dt) == -1 and b"act_dtype" in lib.paro_last_error()
    for adv in (-1, 2):
        assert call(advance=adv) == -1 and b"advance" in lib.paro_last_error()
    assert call(ws_bytes=n - 1) == -1 and b"workspace" in lib.paro_last_error()


def test_sample_params_ranges():
    from paroquant_amd import ops
    p = ops.sample_params("cpu", 0.8, 20, 0.9, 1.2, 7)
    assert p.dtype == torch.uint8 and p.numel() == 24
    raw = p.numpy().tobytes()
    assert np.frombuffer(raw[:12], np.float32).tolist() == [np.float32(0.8), np.float32(0.9), np.float32(1.2)]
    assert np.frombuffer(raw[12:16], np.int32)[0] == 20 and np.frombuffer(raw[16:], np.uint64)[0] == 7
    q = ops.sample_params("cpu", 0.0, -5, 1.0, 1.0, 2 ** 64 - 1, out=p)
    assert q is p and np.frombuffer(p.numpy().tobytes()[16:], np.uint64)[0] == 2 ** 64 - 1
    assert np.frombuffer(ops.sample_params("cpu", 1.0, 10 ** 12, 1.0, 1.0, 0).numpy().tobytes()[12:16], np.int32)[0] == 2 ** 31 - 1
    for bad in (dict(temperature=-0.1), dict(temperature=float("nan")), dict(top_p=0.0), dict(top_p=1.01), dict(top_p=-1.0),
                dict(repetition_penalty=0.0), dict(repetition_penalty=-2.0), dict(top_k=1.5), dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            ops.sample_params("cpu", **bad)


def test_sample_uniform_is_a_counter_based_uniform():
    from paroquant_amd import ops
    n = 1 << 16
    u = np.array([ops.sample_uniform(12345, c) for c in range(n)])
    assert (u >= 0).all() and (u < 1).all()
    assert (u * 2 ** 24 == np.floor(u * 2 ** 24)).all()                       # 24 bits
    assert [ops.sample_uniform(12345, c) for c in range(256)] == u[:256].tolist()              # deterministic
    assert len(set(u[:4096].tolist())) > 4000                                  # differs across counters ...
    other = np.array([ops.sample_uniform(12346, c) for c in range(4096)])
    assert (other != u[:4096]).mean() > 0.99                                   # ... and across seeds
    assert ops.sample_uniform(2 ** 64 - 1, 2 ** 40) != ops.sample_uniform(2 ** 64 - 1, 2 ** 40 + 1)
    assert abs(u.mean() - 0.5) < 0.01
    bins = np.bincount((u * 16).astype(int), minlength=16)
    assert (np.abs(bins - 4096) <= 400).all(), bins


def _hf_keep(logits32, seen, temperature, top_k, top_p, penalty):
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    scores = torch.from_numpy(logits32)[None].clone()
    ids = torch.from_numpy(np.asarray(seen, dtype=np.int64))[None]
    scores = RepetitionPenaltyLogitsProcessor(float(penalty))(ids, scores)
    scores = TemperatureLogitsWarper(float(temperature))(ids, scores)
    if top_k > 0:
        scores = TopKLogitsWarper(int(top_k))(ids, scores)
    scores = TopPLogitsWarper(float(top_p))(ids, scores)
    return torch.isfinite(scores[0]).numpy()


def test_reference_keeps_what_hf_processors_keep():
    """200 seeded cases without (near-)ties at a boundary: the float64 restatement keeps exactly the tokens HF's float32 chain keeps."""
    done, seed = 0, 0
    while done < 200:
        seed += 1
        assert seed < 2000
        rng = np.random.default_rng(seed)
        V = int(rng.integers(2, 600))
        logits = (3.0 * rng.standard_normal(V)).astype(np.float32)
        seen = rng.integers(0, V, size=int(rng.integers(1, 12)))
        temperature = float(rng.choice([0.5, 0.7, 1.0, 1.3]))
        top_k = int(rng.choice([-1, 1, 5, 50, V, V + 1]))
        top_p = float(rng.choice([0.1, 0.5, 0.9, 0.95, 1.0]))
        penalty = float(rng.choice([1.0, 1.1, 1.3, 0.8]))
        ref = sr.Ref(logits, seen, temperature, top_k, top_p, penalty)
        if not ref.decided_set:
            continue
        keep = _hf_keep(logits, seen, temperature, top_k, top_p, penalty)
        assert np.array_equal(keep, ref.keep), (seed, V, temperature, top_k, top_p, penalty, int(keep.sum()), ref.kept)
        done += 1


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("vocab", sr.VOCABS)
def test_kernel_test_inputs_are_decided(vocab, dtype):
    """At most 1 % of the (parameters, counter) cases the GPU test runs at this vocabulary and dtype may be undecided in float64."""
    from paroquant_amd import ops
    logits, hist, _, c0 = sr.kernel_inputs(vocab, dtype)
    total = undecided = 0
    for case, (t, k, p, pen) in enumerate(sr.combos(vocab)):
        ref = sr.Ref(logits.float().numpy(), hist, t, k, p, pen)
        for c in range(c0, c0 + sr.COUNTERS):
            _, decided, _ = ref.pick(ops.sample_uniform(sr.seed_of(case), c))
            total += 1
            undecided += not decided
    assert total == len(sr.combos(vocab)) * sr.COUNTERS
    assert undecided <= 0.01 * total, (undecided, total)
