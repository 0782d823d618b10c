"""Prompt continuation on the GPU (ABI v20): ``paro_attn_prompt`` against a float64 reference and SDPA, and the decode harness'
``prefill(ids, start_pos, chunk_size)`` / ``generate(..., start_pos)`` against one-shot prefill, HF's modelling code, rewinds and graph
replays."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    import paroquant_amd  # noqa: F401
    from paroquant_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _attn_ref(q, kcache, vcache, pos0):
    """float64: row t attends to cache positions 0 .. pos0 + t of KV head h // (H / G)."""
    T, H, hd = q.shape
    G = kcache.size(0)
    n = pos0 + T
    k = kcache[:, :n].double().repeat_interleave(H // G, 0)                     # [H, n, hd]
    v = vcache[:, :, :n].double().transpose(1, 2).repeat_interleave(H // G, 0)  # [H, n, hd]
    s = torch.einsum("thd,hpd->htp", q.double(), k) / math.sqrt(hd)
    keep = torch.arange(n, device=q.device)[None, :] <= (pos0 + torch.arange(T, device=q.device))[:, None]
    s = s.masked_fill(~keep[None], float("-inf"))
    return torch.einsum("htp,hpd->thd", torch.softmax(s, -1), v).reshape(T, H * hd)


# (T, pos0): one row, a block that is not a multiple of the query block, from position 0, crossing / landing on 64-position tiles, long caches
CASES = [(1, 0), (1, 37), (1, 64), (5, 0), (37, 0), (50, 14), (64, 64), (70, 57), (129, 0), (33, 1000), (100, 4000), (4, 4092)]
T_MAX = 4104


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("ratio", [1, 2, 4, 8])
def test_attn_prompt_matches_float64(dev, dtype, hd, ratio):
    from paroquant_amd import ops
    G = 2
    H = G * ratio
    gen = torch.Generator(device=dev).manual_seed(hd * 10 + ratio)
    for T, pos0 in CASES:
        n = pos0 + T
        kc = torch.randn(G, T_MAX, hd, device=dev, generator=gen).to(dtype)
        vc = torch.randn(G, hd, T_MAX, device=dev, generator=gen).to(dtype)
        kc[:, n:] = float("nan")                     # never read
        vc[:, :, n:] = float("nan")
        q = (1.5 * torch.randn(T, H, hd, device=dev, generator=gen)).to(dtype)
        out = ops.attn_prompt(q, kc, vc, pos0)
        again = ops.attn_prompt(q, kc, vc, pos0)
        torch.cuda.synchronize()
        assert out.shape == (T, H * hd) and out.dtype == dtype
        assert torch.isfinite(out.float()).all(), (T, pos0)
        assert torch.equal(out, again), (T, pos0)
        ref = _attn_ref(q, kc, vc, pos0)
        scale = ref.abs().max().item()
        err = (out.double() - ref).abs().max().item()
        assert err <= TOL[dtype] * scale, (T, pos0, err, scale)
        if pos0 == 0:                                # the prompt pass' SDPA over the same rows
            k = kc[:, :T].unsqueeze(0)
            v = vc[:, :, :T].transpose(1, 2).unsqueeze(0)
            sd = torch.nn.functional.scaled_dot_product_attention(q.transpose(0, 1)[None], k, v, is_causal=True, enable_gqa=ratio > 1)
            sd = sd[0].transpose(0, 1).reshape(T, -1)
            assert (out.double() - sd.double()).abs().max().item() <= TOL[dtype] * scale, (T, pos0)


def _ckpt(tmp_path, model_type, hd):
    from tests.hf_ckpt import write_tiny_paro_llama
    path = str(tmp_path / f"{model_type}_{hd}")
    write_tiny_paro_llama(path, hidden=512, inter=1024, heads=8 if hd == 64 else 4, kv_heads=2, layers=2, vocab=200,
                          model_type=model_type, head_dim=hd, seed=3)
    return path


MODELS = [("llama", 64), ("qwen3", 128)]


def _assert_same_state(lm, ref, T, dtype, logits, ref_logits):
    """The caches: the first layer's (the qkv linear of the embeddings) within the kernel test's tolerance of max |ref|; every layer's within
    twice that in norm.  The linears take their kernel by row count (the one-row / skinny GEMV up to 64 rows, the MFMA GEMM above), so a
    chunk's rows are rounded differently from the one-shot prompt's before any attention runs, and the difference compounds through the
    layers: measured on these checkpoints, layer 0 max 5.9e-4 (fp16) / 6.8e-3 (bf16) of max |ref|, layer 1 in norm 2.2e-3 / 1.8e-2 -- the
    same with every prompt row through the skinny route, whichever the attention; a wrong attention is off by tens of percent."""
    scale = ref_logits.abs().max().item()
    assert (logits.float() - ref_logits.float()).abs().max().item() < 2e-2 * scale
    for i, (L, R) in enumerate(zip(lm.layers, ref.layers)):
        for got, want in ((L.kcache[:, :T], R.kcache[:, :T]), (L.vcache[:, :, :T], R.vcache[:, :, :T])):
            got, want = got.double(), want.double()
            assert torch.isfinite(got).all()
            assert ((got - want).norm() / want.norm()).item() <= 2 * TOL[dtype], i
            if i == 0:
                assert (got - want).abs().max().item() <= TOL[dtype] * want.abs().max().item()
    assert int(lm.pos.item()) == int(ref.pos.item()) == T
    assert torch.equal(lm.out_tokens[:T], ref.out_tokens[:T])
    top2 = ref_logits[0].float().topk(2).values
    if (top2[0] - top2[1]).item() > 6e-2 * scale:
        assert int(lm.tok.item()) == int(ref.tok.item())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("model_type, hd", MODELS)
def test_continuation_matches_one_shot(dev, tmp_path, model_type, hd, dtype):
    from paroquant_amd.decoder import ParoDecoderLM
    path = _ckpt(tmp_path, model_type, hd)
    T = 80
    ids = torch.randint(0, 200, (T,), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    one = ParoDecoderLM.from_checkpoint(path, dev, max_positions=128, dtype=dtype)
    ref_logits = one.prefill(ids)
    for a in (1, 17, 64):
        lm = ParoDecoderLM.from_checkpoint(path, dev, max_positions=128, dtype=dtype)
        lm.prefill(ids[:a])
        logits = lm.prefill(ids[a:], start_pos=a)
        torch.cuda.synchronize()
        _assert_same_state(lm, one, T, dtype, logits, ref_logits)
    for C in (1, 7, 16):
        lm = ParoDecoderLM.from_checkpoint(path, dev, max_positions=128, dtype=dtype)
        logits = lm.prefill(ids, chunk_size=C)
        torch.cuda.synchronize()
        _assert_same_state(lm, one, T, dtype, logits, ref_logits)


def _hf(path):
    import paroquant_amd.hf_quantizer  # noqa: F401
    from transformers import AutoModelForCausalLM
    try:
        hf = AutoModelForCausalLM.from_pretrained(path, dtype=torch.float16, device_map={"": "cuda:0"})
    except TypeError:
        hf = AutoModelForCausalLM.from_pretrained(path, torch_dtype=torch.float16, device_map={"": "cuda:0"})
    return hf.eval()


@pytest.mark.parametrize("model_type, hd", MODELS)
def test_multi_turn_matches_hf(dev, tmp_path, model_type, hd):
    from paroquant_amd.decoder import ParoDecoderLM
    path = _ckpt(tmp_path, model_type, hd)
    hf = _hf(path)
    g = torch.Generator(device=dev).manual_seed(11)
    turn1 = torch.randint(0, 200, (11,), device=dev, generator=g)
    turn2 = torch.randint(0, 200, (7,), device=dev, generator=g)
    lm = ParoDecoderLM.from_checkpoint(path, dev, max_positions=64)
    toks, st1 = lm.generate(turn1, 6)
    assert toks.shape == (17,) and torch.equal(toks[:11], turn1) and st1["context_tokens"] == 17
    # turn 2, step by step: the continuation's prefill, then the graph captured by turn 1
    p = len(toks) - 1
    seq = torch.cat([toks, turn2])
    logits = lm.prefill(torch.cat([toks[-1:], turn2]), start_pos=p)
    with torch.no_grad():
        ref = hf(input_ids=seq[None]).logits[0, -1].float()
    scale = ref.abs().max().item()
    assert (logits[0].float() - ref).abs().max().item() < 2e-2 * scale
    top2 = ref.topk(2).values
    if (top2[0] - top2[1]).item() > 6e-2 * scale:
        assert int(lm.tok.item()) == int(ref.argmax().item())
    for step in range(5):
        seq = torch.cat([seq, lm.tok.clone()])
        lm._graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            ref = hf(input_ids=seq[None]).logits[0, -1].float()
        got = lm.logits[0].float()
        assert (got - ref).abs().max().item() < 3e-2 * ref.abs().max().item(), step
        top2 = ref.topk(2).values
        if (top2[0] - top2[1]).item() > 6e-2 * ref.abs().max().item():
            assert int(lm.tok.item()) == int(ref.argmax().item()), step
    seq = torch.cat([seq, lm.tok.clone()])
    # the public recipe returns that whole context
    lm2 = ParoDecoderLM.from_checkpoint(path, dev, max_positions=64)
    t1, _ = lm2.generate(turn1, 6)
    t2, st2 = lm2.generate(torch.cat([t1[-1:], turn2]), 6, start_pos=len(t1) - 1)
    assert torch.equal(t1, toks)
    assert t2.shape == (30,) and st2["context_tokens"] == 30 and st2["prompt_tokens"] == 8 and st2["new_tokens"] == 6
    assert torch.equal(t2[:17], t1) and torch.equal(t2[17:24], turn2)
    assert torch.equal(t2, seq)


@pytest.mark.parametrize("model_type, hd", MODELS)
def test_rewind_never_reads_the_stale_tail(dev, tmp_path, model_type, hd):
    from paroquant_amd.decoder import ParoDecoderLM
    path = _ckpt(tmp_path, model_type, hd)
    g = torch.Generator(device=dev).manual_seed(13)
    ids = torch.randint(0, 200, (20,), device=dev, generator=g)
    b = torch.randint(0, 200, (9,), device=dev, generator=g)
    A = ParoDecoderLM.from_checkpoint(path, dev, max_positions=64)
    B = ParoDecoderLM.from_checkpoint(path, dev, max_positions=64)
    A.prefill(ids[:8])
    A.prefill(ids[8:20], start_pos=8)
    la = A.prefill(b, start_pos=8)
    B.prefill(ids[:8])
    lb = B.prefill(b, start_pos=8)
    torch.cuda.synchronize()
    n = 8 + len(b)
    assert torch.equal(la, lb) and torch.equal(A.tok, B.tok) and int(A.pos.item()) == int(B.pos.item()) == n
    for LA, LB in zip(A.layers, B.layers):
        assert torch.equal(LA.kcache[:, :n], LB.kcache[:, :n])
        assert torch.equal(LA.vcache[:, :, :n], LB.vcache[:, :, :n])


@pytest.mark.parametrize("model_type, hd", MODELS)
def test_graph_replays_after_continuation_match_eager(dev, tmp_path, model_type, hd):
    from paroquant_amd.decoder import ParoDecoderLM
    path = _ckpt(tmp_path, model_type, hd)
    g = torch.Generator(device=dev).manual_seed(17)
    turn1 = torch.randint(0, 200, (9,), device=dev, generator=g)
    turn2 = torch.randint(0, 200, (12,), device=dev, generator=g)
    lm = ParoDecoderLM.from_checkpoint(path, dev, max_positions=64)
    toks, _ = lm.generate(turn1, 4)                  # captures the graph
    graph = lm._graph
    lm.prefill(torch.cat([toks[-1:], turn2]), start_pos=len(toks) - 1)
    tok0, pos0 = lm.tok.clone(), lm.pos.clone()
    replayed = []
    for _ in range(8):
        graph.replay()
        replayed.append(int(lm.tok.item()))
    lm.tok.copy_(tok0)
    lm.pos.copy_(pos0)
    eager = []
    for _ in range(8):
        lm.decode_step()
        eager.append(int(lm.tok.item()))
    assert lm._graph is graph and replayed == eager


def test_continuation_errors(dev, tmp_path):
    from paroquant_amd import ops
    from paroquant_amd.decoder import ParoDecoderLM
    path = _ckpt(tmp_path, "llama", 64)
    lm = ParoDecoderLM.from_checkpoint(path, dev, max_positions=64)
    ids = torch.arange(10, device=dev)
    with pytest.raises(ValueError):
        lm.prefill(ids, start_pos=3)                 # nothing cached yet
    lm.prefill(ids[:5])
    with pytest.raises(ValueError):
        lm.prefill(ids, start_pos=6)                 # beyond the 5 cached positions
    with pytest.raises(ValueError):
        lm.prefill(torch.arange(60, device=dev), start_pos=5)   # 65 > max_positions
    with pytest.raises(ValueError):
        lm.prefill(ids, chunk_size=0)
    with pytest.raises(ValueError):
        lm.prefill(ids, chunk_size=65536)
    with pytest.raises(ValueError):
        lm.generate(ids, 4, start_pos=60)
    q = torch.zeros(4, 2, 256, dtype=torch.float16, device=dev)
    kc = torch.zeros(1, 64, 256, dtype=torch.float16, device=dev)
    vc = torch.zeros(1, 256, 64, dtype=torch.float16, device=dev)
    with pytest.raises(ValueError):
        ops.attn_prompt(q, kc, vc, 0)
    # start_pos 0 without chunking is the fresh prefill, bit for bit
    a = lm.prefill(ids)
    b = ParoDecoderLM.from_checkpoint(path, dev, max_positions=64).prefill(ids, start_pos=0)
    assert torch.equal(a, b)
