"""float64 restatement of the device sampler (``paro_sample_advance``, include/paro_abi.h) and the input list of its tests.

Shared by tests/test_host_sample.py (which checks the restatement against HF's processors and the undecided-share cap on the CPU) and
tests/test_gpu_sample.py (which holds the kernel to it)."""
import numpy as np
import torch

VOCABS = [1, 100, 1000, 32000, 151936]
COUNTERS = 64
MARGIN = 1e-4        # any fp32 summation order with up to ~1000 sequential adds is within 1000 * 2^-24 ~ 6e-5 of the exact sum
TIE_REL = 1e-5


def rounded(x: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dtype)


def make_logits(vocab: int, dtype: torch.dtype, seed: int) -> torch.Tensor:
    """A peaked distribution (a geometric ladder over a random permutation plus noise, rounded to ``dtype``): a handful of tokens carry
    almost all the mass, as a language model's logits do, so that the float64 result is decided for nearly every draw; the tail runs
    into exact ties and, at large vocabularies in fp16, into -inf."""
    rng = np.random.default_rng(seed)
    rank = rng.permutation(vocab).astype(np.float64)
    return rounded(4.0 - 0.75 * rank + 0.2 * rng.standard_normal(vocab), dtype)


def history(vocab: int, logits: torch.Tensor) -> np.ndarray:
    """Seen tokens: duplicates, the most likely token (positive logit), one with a negative logit, and an id outside the vocabulary
    (ignored).  ``out_tokens`` is this list repeated, so the seen set is the same for every counter >= its length."""
    lf = logits.float().numpy()
    top = int(np.argmax(lf))
    neg = np.nonzero(lf < 0)[0]
    pos = np.nonzero(lf > 0)[0]
    h = [top, top, int(neg[0]) if len(neg) else 0, int(pos[-1]) if len(pos) else 0, vocab // 2, top, vocab + 5, min(3, vocab - 1)]
    return np.asarray(h, dtype=np.int64)


def combos(vocab: int):
    """(temperature, top_k, top_p, penalty) of the kernel tests."""
    out = [(0.7, -1, 1.0, 1.0), (1.3, -1, 1.0, 1.0)]
    out += [(1.0, k, 1.0, 1.0) for k in (1, 5, 50, vocab, vocab + 1)]
    out += [(1.0, -1, p, 1.0) for p in (0.1, 0.9, 1.0)]
    out += [(1.0, -1, 1.0, pen) for pen in (1.0, 1.3)]
    out += [(0.8, 20, 0.9, 1.2)]
    return out


class Ref:
    """Steps 1-4 of the sampler for one (logits, seen set, parameters) in float64; :meth:`pick` is steps 5-6 for one u."""

    def __init__(self, logits, seen, temperature, top_k, top_p, penalty):
        s = np.asarray(logits, dtype=np.float64).copy()
        V = len(s)
        seen = np.unique([t for t in np.asarray(seen, dtype=np.int64).tolist() if 0 <= t < V]).astype(np.int64)
        if len(seen):
            s[seen] = np.where(s[seen] > 0, s[seen] / penalty, s[seen] * penalty)
        self.V, self.greedy, self.decided_set = V, temperature == 0, True
        if self.greedy:
            self.scores, self.token = s, int(np.argmax(s))
            self.keep = np.zeros(V, bool)
            self.keep[self.token] = True
            self.kept, self.boundary = 1, s[self.token]
            return
        s = s / temperature
        keep = np.ones(V, bool)
        self.boundary = -np.inf
        if 0 < top_k < V:
            srt = np.sort(s)[::-1]
            kth, nxt = srt[top_k - 1], srt[top_k]
            keep = s >= kth
            self.boundary = kth
            if not (nxt == kth or abs(kth - nxt) > TIE_REL * max(abs(kth), abs(nxt))):
                self.decided_set = False
        M = s[keep].max()
        with np.errstate(invalid="ignore"):
            e = np.where(keep, np.exp(s - M), 0.0)
        if top_p < 1.0:
            idx = np.nonzero(keep)[0]
            order = idx[np.argsort(-s[idx], kind="stable")]
            cum = np.cumsum(e[order])
            total = cum[-1]
            j = min(int(np.searchsorted(cum, top_p * total, side="left")), len(order) - 1)
            self.boundary = s[order[j]]
            keep = keep & (s >= self.boundary)
            # the decision changes only where a whole group of equal scores ends: the cumulative masses there
            with np.errstate(invalid="ignore"):
                ends = np.nonzero(np.diff(s[order]) != 0)[0]
            edges = np.concatenate([cum[ends], cum[-1:]])
            if np.min(np.abs(edges - top_p * total)) <= MARGIN * total:
                self.decided_set = False
            e = np.where(keep, e, 0.0)
        self.scores, self.keep, self.kept = s, keep, int(keep.sum())
        self.cum = np.cumsum(e)             # index order
        self.Z = self.cum[-1]

    def pick(self, u: float):
        """(token, decided, neighbours): the lowest index whose cumulative kept mass exceeds u Z; ``neighbours`` are the kept indices
        next to it, one of which an undecided draw may land on."""
        if self.greedy:
            return self.token, True, (self.token,)
        x = float(u) * self.Z
        i = int(np.searchsorted(self.cum, x, side="right"))
        kept_idx = np.nonzero(self.keep)[0]
        if i >= self.V or not self.keep[i]:
            i = int(kept_idx[min(np.searchsorted(kept_idx, i), len(kept_idx) - 1)])
        below = self.cum[i - 1] if i > 0 else 0.0
        decided = self.decided_set and x - below > MARGIN * self.Z and self.cum[i] - x > MARGIN * self.Z
        j = int(np.searchsorted(kept_idx, i))
        near = tuple(int(kept_idx[k]) for k in (j - 1, j, j + 1) if 0 <= k < len(kept_idx))
        return i, bool(decided), near


def kernel_inputs(vocab: int, dtype: torch.dtype):
    """(logits, history, out_tokens, first counter) of the parametrised kernel test."""
    logits = make_logits(vocab, dtype, seed=vocab + (1 if dtype == torch.bfloat16 else 0))
    hist = history(vocab, logits)
    out_tokens = np.tile(hist, (len(hist) + COUNTERS + len(hist) - 1) // len(hist) + 1)[: len(hist) + COUNTERS]
    return logits, hist, out_tokens, len(hist)


def seed_of(case: int) -> int:
    return 1000 + 17 * case
