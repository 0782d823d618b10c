#!/usr/bin/env python3
"""Prompt-continuation attention (ops.attn_prompt, ABI v20) on Qwen3-4B heads (32 query / 8 KV heads, head_dim 128), fp16 and bf16:
  kernel  the kernel against the prompt pass' SDPA call at pos0 = 0 (T = 128, 512, 2048), and the kernel alone at pos0 = 1024, 4096 (T = 128);
          us per call = one timed repetition of --calls back-to-back calls / --calls (device events)
  e2e     ParoDecoderLM.random("qwen3-4b") time to first token of a 128-token turn behind 1024 cached positions
          (prefill(turn, start_pos=1024)) against a fresh prefill of all 1152 tokens and a fresh 128-token prompt
Every number is the median of --reps timed repetitions after --warmup, with min and max; each line names the box.
    python tools/bench_prompt_attn.py [--out profiles/r07_prompt_attn.jsonl] [--reps 7]"""
import argparse, json, os, socket, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from paroquant_amd import ops

H, KV, HD = 32, 8, 128


def stats(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(np.min(xs)), 3), "max": round(float(np.max(xs)), 3), "reps": len(xs)}


def time_calls(fn, calls, reps, warmup):
    """us per call: each repetition times `calls` back-to-back calls between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return out


def time_host(fn, reps, warmup):
    """ms per call: host clock around one call that ends in a device synchronise."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_prompt_attn.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be >= 5")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    props = torch.cuda.get_device_properties(dev)
    box = {"host": socket.gethostname(), "gpu": torch.cuda.get_device_name(dev), "arch": props.gcnArchName, "cus": props.multi_processor_count}
    lines = []

    def emit(d):
        d.update(box)
        lines.append(d)
        print(json.dumps(d), flush=True)

    sdpa = torch.nn.functional.scaled_dot_product_attention
    T_max = 4096 + 128 + 8
    g = torch.Generator(device=dev).manual_seed(0)
    for dt in (torch.float16, torch.bfloat16):
        name = "fp16" if dt == torch.float16 else "bf16"
        kc = torch.randn(KV, T_max, HD, device=dev, generator=g).to(dt)
        vc = torch.randn(KV, HD, T_max, device=dev, generator=g).to(dt)
        for T in (128, 512, 2048):
            q = torch.randn(T, H, HD, device=dev, generator=g).to(dt)
            k = kc[:, :T].transpose(0, 1).contiguous()          # [T, KV, hd]: what prompt_qkv_post hands the SDPA call
            v = vc[:, :, :T].permute(2, 0, 1).contiguous()
            run_k = lambda: ops.attn_prompt(q, kc, vc, 0)
            run_s = lambda: sdpa(q.transpose(0, 1)[None], k.transpose(0, 1)[None], v.transpose(0, 1)[None], is_causal=True,
                                 enable_gqa=True)[0].transpose(0, 1).reshape(T, -1)
            err = (run_k().float() - run_s().float()).abs().max().item()
            tk, ts = stats(time_calls(run_k, a.calls, a.reps, a.warmup)), stats(time_calls(run_s, a.calls, a.reps, a.warmup))
            emit({"what": "attn_prompt vs sdpa at pos0 = 0", "dtype": name, "T": T, "pos0": 0, "heads": H, "kv_heads": KV, "head_dim": HD,
                  "kernel_us": tk, "sdpa_us": ts, "sdpa_over_kernel": round(ts["median"] / tk["median"], 3), "max_abs_diff": err})
        for pos0 in (1024, 4096):
            T = 128
            q = torch.randn(T, H, HD, device=dev, generator=g).to(dt)
            tk = stats(time_calls(lambda: ops.attn_prompt(q, kc, vc, pos0), a.calls, a.reps, a.warmup))
            n = pos0 + T
            # what the causal product must at least read: K and V of positions 0 .. pos0 + T - 1, q and out
            nbytes = 2 * KV * n * HD * 2 + 2 * T * H * HD * 2
            emit({"what": "attn_prompt continuation", "dtype": name, "T": T, "pos0": pos0, "heads": H, "kv_heads": KV, "head_dim": HD,
                  "kernel_us": tk, "min_bytes": nbytes, "GBps_at_median": round(nbytes / tk["median"] / 1e3, 1)})
        del kc, vc

    if not a.skip_e2e:
        from paroquant_amd.decoder import ParoDecoderLM
        lm = ParoDecoderLM.random("qwen3-4b", dev, max_positions=1152 + 64)
        vocab = lm.cfg.vocab
        ids = torch.randint(0, vocab, (1152,), device=dev, generator=g)
        hist, turn = ids[:1024], ids[1024:]
        fresh128 = stats(time_host(lambda: lm.prefill(turn), a.reps, a.warmup))
        fresh1152 = stats(time_host(lambda: lm.prefill(ids), a.reps, a.warmup))
        lm.prefill(hist)
        torch.cuda.synchronize()
        # every repetition rewrites positions 1024 .. 1151 behind the same 1024-position history
        cont = stats(time_host(lambda: lm.prefill(turn, start_pos=1024), a.reps, a.warmup))
        emit({"what": "time to first token, qwen3-4b (36 layers, synthetic weights, fp16)", "unit": "ms",
              "turn_128_after_1024_cached": cont, "fresh_prefill_1152": fresh1152, "fresh_prompt_128": fresh128,
              "continuation_over_fresh_128": round(cont["median"] / fresh128["median"], 3),
              "continuation_over_fresh_1152": round(cont["median"] / fresh1152["median"], 3)})

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
