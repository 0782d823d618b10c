"""The device sampler (``paro_sample_advance``, csrc/sample.hip) against the float64 restatement of tests/sample_ref.py, and sampled
generation in the decode harness.  Nothing here is statistical: the draw ``u`` is host-computable (``ops.sample_uniform``), so the
expected token of every decided case is known exactly."""
import numpy as np
import pytest
import torch

from tests import sample_ref as sr

pytestmark = pytest.mark.gpu

SAMPLED = dict(temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.2, seed=7)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    import paroquant_amd  # noqa: F401
    from paroquant_amd import _native
    _native.load()
    return torch.device("cuda:0")


class Runner:
    """One vocabulary's device buffers; :meth:`run` returns (token, pos after, stats [4] float32 bits as numpy) per counter."""

    def __init__(self, dev, logits, out_tokens):
        from paroquant_amd import ops
        self.ops, self.dev = ops, dev
        self.logits = logits.to(dev)
        self.ws = ops.sample_workspace(dev, logits.numel())
        self.tok = torch.zeros(1, dtype=torch.long, device=dev)
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.out = None if out_tokens is None else torch.from_numpy(np.asarray(out_tokens, dtype=np.int64)).to(dev)
        self.prm = None

    def run(self, counters, advance=False, token_in=0, **params):
        self.prm = self.ops.sample_params(self.dev, out=self.prm, **params)
        n = len(counters)
        toks = torch.zeros(n, dtype=torch.long, device=self.dev)
        poss = torch.zeros(n, dtype=torch.int32, device=self.dev)
        stats = torch.zeros(n, 4, dtype=torch.float32, device=self.dev)
        for i, c in enumerate(counters):
            self.pos.fill_(c - 1 if advance else c)
            self.tok.fill_(token_in)
            self.ops.sample_advance(self.logits, self.prm, self.tok, self.pos, self.out, self.ws, advance=advance)
            toks[i:i + 1] = self.tok
            poss[i:i + 1] = self.pos
            stats[i] = self.ws[:16].view(torch.float32)
        torch.cuda.synchronize()
        return toks.cpu().numpy(), poss.cpu().numpy(), stats.cpu().numpy()


def _check(ref, toks, stats, seed, counters, what):
    """Decided draws match exactly (token, kept count, u); an undecided one lands beside the float64 pick.  Returns the undecided count."""
    from paroquant_amd import ops
    undecided = 0
    for tok, st, c in zip(toks, stats, counters):
        u = ops.sample_uniform(seed, c)
        want, decided, near = ref.pick(u)
        print(what, "ctr", c, "u", u, "token", int(tok), "ref", want, "decided", decided, "kept", st[0], ref.kept, "Z", st[2])
        assert np.float32(st[3]) == np.float32(u), (what, c)
        assert 0 <= tok < ref.V, (what, c)
        if ref.decided_set:
            assert int(st[0]) == ref.kept, (what, c, st[0], ref.kept)
            assert ref.keep[tok], (what, c, int(tok))
        if decided:
            assert int(tok) == want, (what, c, int(tok), want)
        else:
            undecided += 1
            if ref.decided_set:
                assert int(tok) in near, (what, c, int(tok), near)
    return undecided


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("vocab", sr.VOCABS)
def test_sampler_matches_float64(dev, vocab, dtype):
    logits, hist, out_tokens, c0 = sr.kernel_inputs(vocab, dtype)
    r = Runner(dev, logits, out_tokens)
    counters = list(range(c0, c0 + sr.COUNTERS))
    total = undecided = 0
    for case, (t, k, p, pen) in enumerate(sr.combos(vocab)):
        seed = sr.seed_of(case)
        toks, poss, stats = r.run(counters, temperature=t, top_k=k, top_p=p, repetition_penalty=pen, seed=seed)
        assert (poss == np.asarray(counters)).all()                       # advance = 0 leaves the position alone
        ref = sr.Ref(logits.float().numpy(), hist, t, k, p, pen)
        undecided += _check(ref, toks, stats, seed, counters, (vocab, str(dtype), t, k, p, pen))
        total += len(counters)
        zref = np.float32(ref.Z)
        assert np.allclose(stats[:, 2], zref, rtol=1e-5), (stats[0, 2], zref)
        if ref.decided_set and ref.boundary > -np.inf:
            assert np.allclose(stats[:, 1], ref.boundary, rtol=1e-6), (stats[0, 1], ref.boundary)
    assert undecided <= 0.01 * total, (undecided, total)
    assert torch.equal(r.out, torch.from_numpy(out_tokens).to(dev))         # advance = 0 writes no history
    n = r.ws.numel()
    assert not r.ws[n - (vocab + 15) // 16 * 16:].any()                      # the seen-set flags are clear again after every call


def test_top_k_1_is_argmax_and_temperature_0_is_penalised_argmax(dev):
    for dtype in (torch.float16, torch.bfloat16):
        for vocab in (100, 32000):
            rng = np.random.default_rng(vocab)
            x = 2.0 * rng.standard_normal(vocab)
            logits = sr.rounded(x, dtype)
            lf = logits.float().numpy().copy()
            top = int(np.argmax(lf))
            lf[top] = lf[top] + 1.0                                         # a unique maximum that stays one after rounding
            logits = sr.rounded(lf, dtype)
            r = Runner(dev, logits, np.asarray([top, top, 1], dtype=np.int64))
            toks, _, stats = r.run([3, 4, 5], temperature=1.0, top_k=1, top_p=1.0, repetition_penalty=1.0, seed=3)
            assert (toks == int(torch.argmax(logits.to(dev)).item())).all() and (stats[:, 0] == 1).all()
            # temperature 0 with a penalty: the argmax moves off the penalised maximum when the runner-up overtakes it
            lf2 = logits.float().numpy().copy()
            second = int(np.argsort(-lf2)[1])
            lf2[top] = lf2[second] * 1.2 if lf2[second] > 0 else lf2[top]
            logits2 = sr.rounded(lf2, dtype)
            r2 = Runner(dev, logits2, np.asarray([top, top, 1], dtype=np.int64))
            toks, _, stats = r2.run([3, 4], temperature=0.0, top_k=-1, top_p=1.0, repetition_penalty=1.3, seed=3)
            ref = sr.Ref(logits2.float().numpy(), [top, top, 1], 0.0, -1, 1.0, 1.3)
            assert (toks == ref.token).all(), (toks, ref.token)
            assert ref.token != top or lf2[second] <= 0
            assert stats[0, 3] == np.float32(r2.ops.sample_uniform(3, 3))


def test_all_equal_logits_and_lowest_index_ties(dev):
    from paroquant_amd import ops
    for vocab in (7, 64, 1000, 4097):
        r = Runner(dev, torch.full((vocab,), 1.5, dtype=torch.float16), None)
        counters = list(range(40))
        toks, _, stats = r.run(counters, temperature=0.9, top_k=5, top_p=0.5, repetition_penalty=1.0, seed=11)
        assert (stats[:, 0] == vocab).all()                                  # ties at both boundaries are kept whole
        for tok, c in zip(toks, counters):
            x = ops.sample_uniform(11, c) * vocab
            want = int(np.floor(x))
            decided = min(x - want, want + 1 - x) > sr.MARGIN * vocab
            assert tok == want or (not decided and abs(int(tok) - want) <= 1), (vocab, c, tok, x)
        toks, _, _ = r.run([0, 1], temperature=0.0, top_k=-1, top_p=1.0, repetition_penalty=1.0, seed=11)
        assert (toks == 0).all()                                             # argmax: lowest index on ties


def test_single_finite_logit_and_boundary_ties(dev):
    for dtype in (torch.float16, torch.bfloat16):
        for vocab in (1, 3, 70, 5000):
            x = torch.full((vocab,), float("-inf"), dtype=dtype)
            x[vocab - 1 - vocab // 3] = -2.0
            r = Runner(dev, x, None)
            for params in (dict(temperature=1.0, top_k=-1, top_p=1.0), dict(temperature=0.7, top_k=4, top_p=0.8), dict(temperature=0.0, top_k=-1, top_p=1.0)):
                toks, _, stats = r.run(list(range(8)), repetition_penalty=1.0, seed=5, **params)
                assert (toks == vocab - 1 - vocab // 3).all(), (vocab, params, toks)
                assert (stats[:, 2] == 1.0).all()
    # top-k boundary inside a group of equal scores: the whole group stays; top-p likewise
    lf = np.full(300, -8.0)
    lf[[5, 17, 40]] = [3.0, 2.0, 2.0]
    lf[[100, 200, 250, 299]] = 1.0
    r = Runner(dev, sr.rounded(lf, torch.float16), None)
    counters = list(range(64))
    for k, p, kept in ((2, 1.0, 3), (4, 1.0, 7), (5, 1.0, 7), (-1, 0.6, 3), (-1, 0.4, 1), (-1, 0.5, 3), (3, 0.95, 3), (7, 0.9, 7)):
        toks, _, stats = r.run(counters, temperature=1.0, top_k=k, top_p=p, repetition_penalty=1.0, seed=9)
        ref = sr.Ref(lf, [], 1.0, k, p, 1.0)
        assert ref.kept == kept and ref.decided_set, (k, p, ref.kept)
        assert _check(ref, toks, stats, 9, counters, ("ties", k, p)) <= 2


def test_advance_history_and_positions(dev):
    vocab = 1000
    logits, hist, _, _ = sr.kernel_inputs(vocab, torch.float16)
    lf = logits.float().numpy()
    params = dict(temperature=0.9, top_k=-1, top_p=1.0, repetition_penalty=1.5, seed=21)
    out = np.zeros(16, dtype=np.int64)
    out[:4] = [int(np.argsort(-lf)[1]), 7, 7, 9]
    top = int(np.argmax(lf))
    # advance = 1 at p = 4: out_tokens[4] = token (the most likely token, which the penalty must then see), ctr = 5, pos -> 5
    r = Runner(dev, logits, out)
    toks, poss, stats = r.run([5], advance=True, token_in=top, **params)
    assert poss[0] == 5 and int(r.out[4].item()) == top and torch.equal(r.out[:4].cpu(), torch.from_numpy(out[:4]))
    assert not r.out[5:].any()
    ref = sr.Ref(lf, list(out[:4]) + [top], 0.9, -1, 1.0, 1.5)
    _check(ref, toks, stats, 21, [5], "advance")
    assert np.allclose(stats[0, 2], ref.Z, rtol=1e-5)                       # Z shows that the token written by this call was penalised
    assert not np.allclose(ref.Z, sr.Ref(lf, list(out[:4]), 0.9, -1, 1.0, 1.5).Z, rtol=1e-3)
    # advance = 0 at p = 4: nothing written, ctr = 4
    r = Runner(dev, logits, out)
    toks, poss, stats = r.run([4], advance=False, token_in=top, **params)
    assert poss[0] == 4 and torch.equal(r.out.cpu(), torch.from_numpy(out))
    ref0 = sr.Ref(lf, list(out[:4]), 0.9, -1, 1.0, 1.5)
    assert np.allclose(stats[0, 2], ref0.Z, rtol=1e-5) and stats[0, 3] == np.float32(r.ops.sample_uniform(21, 4))
    _check(ref0, toks, stats, 21, [4], "no advance")
    # no history array; positions outside it (both sides): nothing written, the seen set stops at the array's end
    r = Runner(dev, logits, None)
    toks, poss, stats = r.run([3, 50], advance=True, token_in=top, **params)
    assert list(poss) == [3, 50] and np.allclose(stats[:, 2], sr.Ref(lf, [], 0.9, -1, 1.0, 1.5).Z, rtol=1e-5)
    r = Runner(dev, logits, out)
    toks, poss, stats = r.run([17, 40, 0], advance=True, token_in=top, **params)      # p = 16, 39, -1
    assert list(poss) == [17, 40, 0] and torch.equal(r.out.cpu(), torch.from_numpy(out))
    assert np.allclose(stats[:2, 2], sr.Ref(lf, list(out), 0.9, -1, 1.0, 1.5).Z, rtol=1e-5)
    assert np.allclose(stats[2, 2], sr.Ref(lf, [], 0.9, -1, 1.0, 1.5).Z, rtol=1e-5)
    assert (toks >= 0).all() and (toks < vocab).all()


def test_same_call_50_times_same_bits(dev):
    logits, hist, out_tokens, c0 = sr.kernel_inputs(151936, torch.bfloat16)
    r = Runner(dev, logits, out_tokens)
    toks, _, stats = r.run([c0 + 3] * 50, temperature=1.1, top_k=40, top_p=0.9, repetition_penalty=1.2, seed=99)
    assert (toks == toks[0]).all()
    assert (stats.view(np.uint32) == stats.view(np.uint32)[0]).all()


# ------------------------------------------------------------------------------------------------------------ the decode harness
def _ckpt(tmp_path, model_type, hd):
    from tests.hf_ckpt import write_tiny_paro_llama
    path = str(tmp_path / f"{model_type}_{hd}")
    write_tiny_paro_llama(path, hidden=512, inter=1024, heads=8 if hd == 64 else 4, kv_heads=2, layers=2, vocab=200,
                          model_type=model_type, head_dim=hd, seed=3)
    return path


def _eager_with_logits(lm, ids, n_new, start_pos=0, **params):
    """generate(use_graph=False) step by step, keeping every step's logits: (tokens, [logits per generated position])."""
    from paroquant_amd import ops
    lm._sampler(params["temperature"], params["top_k"], params["top_p"], params["repetition_penalty"], params["seed"])
    logits = [lm.prefill(ids, start_pos=start_pos).view(-1).float().cpu().numpy()]
    ops.sample_advance(torch.from_numpy(logits[0]).to(lm.device, lm.dtype), lm.sample_prm, lm.tok, lm.pos, lm.out_tokens, lm.sample_ws, advance=False)
    for _ in range(n_new - 1):
        lm.decode_step(True)
        logits.append(lm.logits.view(-1).float().cpu().numpy())
    lm.out_tokens.index_copy_(0, lm.pos.long(), lm.tok)
    return lm.out_tokens[: start_pos + ids.numel() + n_new].cpu().numpy(), logits


@pytest.mark.parametrize("model_type, hd", [("llama", 64), ("qwen3", 128)])
def test_sampled_generate_graph_equals_eager_and_follows_the_reference(dev, tmp_path, model_type, hd):
    from paroquant_amd import ops
    from paroquant_amd.decoder import ParoDecoderLM
    path = _ckpt(tmp_path, model_type, hd)
    ids = torch.randint(0, 200, (12,), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    n_new, T = 24, 12
    lm = ParoDecoderLM.from_checkpoint(path, dev, max_positions=128)
    greedy, _ = lm.generate(ids, n_new)
    assert lm._graph is not None and lm._graph_sampled is None              # the defaults are the greedy route
    ref_lm = ParoDecoderLM.from_checkpoint(path, dev, max_positions=128)
    ref_lm.prefill(ids)
    for _ in range(n_new - 1):
        ref_lm.decode_step()
    ref_lm.out_tokens.index_copy_(0, ref_lm.pos.long(), ref_lm.tok)
    assert torch.equal(greedy, ref_lm.out_tokens[: T + n_new])
    assert ref_lm.sample_ws is None

    graph, _ = lm.generate(ids, n_new, **SAMPLED)
    g = lm._graph_sampled
    assert g is not None
    eager_lm = ParoDecoderLM.from_checkpoint(path, dev, max_positions=128)
    eager, _ = eager_lm.generate(ids, n_new, use_graph=False, **SAMPLED)
    assert eager_lm._graph_sampled is None and torch.equal(graph, eager)
    assert not torch.equal(graph, greedy)
    # every token against the float64 restatement on the eager run's logits
    toks, logits = _eager_with_logits(ParoDecoderLM.from_checkpoint(path, dev, max_positions=128), ids, n_new, **SAMPLED)
    assert (toks == eager.cpu().numpy()).all()
    for i in range(n_new):
        ctr = T + i
        ref = sr.Ref(logits[i], toks[:ctr], 0.8, 20, 0.9, 1.2)
        want, decided, _ = ref.pick(ops.sample_uniform(7, ctr))
        print("step", i, "token", toks[ctr], "ref", want, "decided", decided, "kept", ref.kept)
        assert not ref.decided_set or ref.keep[toks[ctr]], i
        assert not decided or toks[ctr] == want, (i, toks[ctr], want)
    # seeds: another seed another sequence, the same seed the same one
    other, _ = lm.generate(ids, n_new, **{**SAMPLED, "seed": 8})
    again, _ = lm.generate(ids, n_new, **SAMPLED)
    assert not torch.equal(other, graph) and torch.equal(again, graph)
    # other parameters through the SAME graph: top_k = 1 without a penalty is the greedy sequence
    k1, _ = lm.generate(ids, n_new, temperature=1.0, top_k=1, seed=3)
    assert lm._graph_sampled is g
    assert torch.equal(k1, greedy)
    pen, _ = lm.generate(ids, n_new, temperature=0.0, repetition_penalty=1.3)
    pen_eager, _ = eager_lm.generate(ids, n_new, use_graph=False, temperature=0.0, repetition_penalty=1.3)
    assert lm._graph_sampled is g and torch.equal(pen, pen_eager)
    # and the greedy route is still the parent's
    again, _ = lm.generate(ids, n_new)
    assert torch.equal(again, greedy)


def test_multi_turn_penalises_the_first_turn(dev, tmp_path):
    from paroquant_amd import ops
    from paroquant_amd.decoder import ParoDecoderLM
    path = _ckpt(tmp_path, "qwen3", 128)
    g = torch.Generator(device=dev).manual_seed(6)
    turn1, turn2 = torch.randint(0, 200, (9,), device=dev, generator=g), torch.randint(0, 200, (5,), device=dev, generator=g)
    lm = ParoDecoderLM.from_checkpoint(path, dev, max_positions=128)
    params = dict(temperature=0.0, top_k=-1, top_p=1.0, repetition_penalty=50.0, seed=1)
    toks1, _ = lm.generate(turn1, 6, **params)
    start = len(toks1) - 1
    ids2 = torch.cat([toks1[-1:], turn2])
    toks2, _ = lm.generate(ids2, 8, start_pos=start, **params)
    assert torch.equal(toks2[: len(toks1)], toks1)
    # the same second turn step by step, with every step's logits: the choice is the argmax of the scores penalised over BOTH turns
    lm2 = ParoDecoderLM.from_checkpoint(path, dev, max_positions=128)
    lm2.generate(turn1, 6, use_graph=False, **params)
    toks, logits = _eager_with_logits(lm2, ids2, 8, start_pos=start, **params)
    assert (toks == toks2.cpu().numpy()).all()
    first_turn_only = 0
    for i in range(8):
        ctr = start + len(ids2) + i
        ref = sr.Ref(logits[i], toks[:ctr], 0.0, -1, 1.0, 50.0)
        srt = np.sort(ref.scores)
        if srt[-1] - srt[-2] > 1e-5 * max(abs(srt[-1]), abs(srt[-2])):
            assert toks[ctr] == ref.token, i
        unpenalised_turn1 = sr.Ref(logits[i], toks[start + 1:ctr], 0.0, -1, 1.0, 50.0)
        first_turn_only += unpenalised_turn1.token != ref.token
    assert first_turn_only > 0        # forgetting the first turn would have chosen differently somewhere


def test_qwen35_sampled_generate(dev):
    from paroquant_amd import ops
    from paroquant_amd.decoder_qwen35 import ParoQwen35DecoderLM, Qwen35Config
    cfg = Qwen35Config(512, 1024, 4, 2, 256, 2, 4, 4, 640, ["linear_attention", "linear_attention", "linear_attention", "full_attention"], max_positions=96)
    lm = ParoQwen35DecoderLM.random(cfg, dev, seed=11)
    ids = torch.randint(0, 640, (10,), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    greedy, _ = lm.generate(ids, 12)
    assert lm._graph_sampled is None
    graph, _ = lm.generate(ids, 12, **SAMPLED)
    assert lm._graph_sampled is not None
    eager_lm = ParoQwen35DecoderLM.random(cfg, dev, seed=11)
    eager, _ = eager_lm.generate(ids, 12, use_graph=False, **SAMPLED)
    assert torch.equal(graph, eager) and not torch.equal(graph, greedy)
    again, _ = lm.generate(ids, 12)
    assert torch.equal(again, greedy)
    # step by step against the float64 restatement
    lm3 = ParoQwen35DecoderLM.random(cfg, dev, seed=11)
    lm3.sample_ws = ops.sample_workspace(dev, 640)
    lm3.sample_prm = ops.sample_params(dev, **SAMPLED)
    logits = [lm3.prefill(ids, use_graph=False).view(-1).float().cpu().numpy()]
    ops.sample_advance(torch.from_numpy(logits[0]).to(dev, lm3.dtype), lm3.sample_prm, lm3.tok, lm3.pos, lm3.out_tokens, lm3.sample_ws, advance=False)
    for _ in range(11):
        lm3.decode_step(True)
        logits.append(lm3.logits.view(-1).float().cpu().numpy())
    lm3.out_tokens.index_copy_(0, lm3.pos.long(), lm3.tok)
    toks = lm3.out_tokens[:22].cpu().numpy()
    assert (toks == eager.cpu().numpy()).all()
    for i in range(12):
        ref = sr.Ref(logits[i], toks[:10 + i], 0.8, 20, 0.9, 1.2)
        want, decided, _ = ref.pick(ops.sample_uniform(7, 10 + i))
        assert not decided or toks[10 + i] == want, (i, toks[10 + i], want)
