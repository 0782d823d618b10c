#!/usr/bin/env python3
"""The host-only queries of the GEMV launcher (csrc/gemv.hip), recorded from ONE build of the library so that a later build can be
held against them answer for answer: `paro_gemv_launch_shape` (return code and its four outputs), `paro_linear_workspace_bytes`,
`paro_gemv_parts_count` and `paro_attn_tail_supported` over bench.py's model shapes (dense at TP 1 / 2 / 4 / 8, the hybrids) and the ad-hoc
shapes of tests/test_host_logic.py, at 1..64 rows, under automatic and explicit knobs and the layer variants (group size, krot, bias,
launch hint).  No device is touched.  Record from a build of the sources whose behaviour is to be KEPT -- the parent of a refactor, made
into its own directory -- never from the code under test:
    make -C paroquant_amd/csrc OUT=$PWD/paroquant_amd/_lib_parent        # in a checkout of the parent commit
    PARO_LIB_DIR=_lib_parent python tests/golden/make_gemv_host_table.py
tests/test_host_logic.py::test_gemv_host_queries_match_the_recorded_table replays every row."""
import ctypes
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

ROWS = (1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 24, 32, 33, 48, 64)
HINT = 2 | (2 << 8) | (8 << 16)                     # a packed launch hint: 2 tiles per wave, 2 K-slices, 8 waves
# knob sets (tiles per wave, ksplit, waves, mode): all auto; each explicit mode; ksplit 1 / 4; each tiles-per-wave; 4 / 16 waves
KNOBS = [(0, 0, 0, -1), (0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 0, 3), (0, 1, 0, -1), (0, 4, 0, -1),
         (1, 0, 0, -1), (2, 0, 0, -1), (4, 0, 0, -1), (8, 0, 0, -1), (0, 0, 4, -1), (0, 0, 16, -1)]
# layer variants (group size, krot, bias, launch hint) -> knob sets recorded for them: the plain layer under every knob set, each
# single deviation under the automatic knobs and one of each kind of explicit knob, all deviations at once under the automatic knobs
# (the full cross product would not fit the 256 KB the table may take; every shape and every row count is kept)
SOME = [0, 1, 3, 5, 9, 11]
VARIANTS = [((128, 8, 0, 0), list(range(len(KNOBS)))), ((64, 8, 0, 0), SOME), ((128, 16, 0, 0), SOME), ((128, 8, 1, 0), SOME),
            ((128, 8, 0, HINT), SOME), ((64, 16, 1, HINT), [0])]
MAX_POSITIONS = 4096


def shapes():
    """Every distinct (K, partition sizes), in a fixed order."""
    import bench
    out = []
    for tp in (1, 2, 4, 8):
        for m in bench.MODELS:
            if bench.shard_error(m, tp) is None:
                out += [(K, tuple(s)) for _, K, s, _ in bench.layer_shapes(m, tp)]
        for m in bench.HYBRID:
            if bench.shard_error(m, tp) is None:
                for full in (False, True):
                    out += [(K, tuple(s)) for _, K, s, _ in bench.hybrid_layer_shapes(m, full, tp)]
    out += [(8192, (7168, 7168)), (8192, (2048, 256, 256)), (1536, (512,)), (4096, (1024,))]
    return list(dict.fromkeys(out))


def attn_geometry(N):
    """(n_heads, n_kv_heads, head_dim) asked of paro_attn_tail_supported: the one N implies with 8 KV heads of 128, else a fixed one."""
    if N % 128 == 0 and N // 128 > 16:
        return N // 128 - 16, 8, 128
    return 32, 8, 128


def evaluate(lib, nat, shape_tab, idx):
    """Answers of the library for rows `idx` = [shape, rows, group size, krot, bias, hint, tpw, ksplit, waves, mode]:
    [rc, tpw, ksplit, waves, mode, workspace bytes, parts count, attention tail supported] per row."""
    out = np.zeros((len(idx), 8), dtype=np.int64)
    cache = {}
    for r, (si, rows, gs, krot, bias, hint, tpw, ks, wv, mode) in enumerate(idx.tolist()):
        K, n_parts = int(shape_tab[si, 0]), int(shape_tab[si, 1])
        sizes = [int(v) for v in shape_tab[si, 2:2 + n_parts]]
        d = nat.ParoLinearDesc()
        d.K, d.N, d.n_parts, d.krot, d.act_dtype, d.wq_order, d.group_size, d.launch_hint = K, sum(sizes), n_parts, krot, nat.DTYPE_F16, 0, gs, hint
        for i, s in enumerate(sizes):
            d.part_cols[i] = s
        for f in ("wq", "sz", "rot", "pairs", "theta", "channel_scales") + (("bias",) if bias else ()):
            setattr(d, f, 0x1000)          # never dereferenced on the host
        o = [ctypes.c_int(v) for v in (tpw, ks, wv, mode)]
        rc = lib.paro_gemv_launch_shape(ctypes.byref(d), rows, *[ctypes.byref(v) for v in o])
        key = (si, rows, gs, krot, bias, hint)
        if key not in cache:
            cache[key] = (lib.paro_linear_workspace_bytes(ctypes.byref(d), rows), lib.paro_gemv_parts_count(ctypes.byref(d)),
                          lib.paro_attn_tail_supported(ctypes.byref(d), *attn_geometry(d.N), MAX_POSITIONS))
        out[r] = (rc, *[v.value for v in o], *cache[key])
    return out


def main():
    from paroquant_amd import _native as nat
    for knob in ("PARO_SHARED_ROT_MIN_ROWS", "PARO_SHR_SELF"):
        if knob in os.environ:
            raise SystemExit(f"{knob} is set: it changes the answers")
    lib = nat.load()
    sh = shapes()
    shape_tab = np.zeros((len(sh), 10), dtype=np.int32)
    for i, (K, sizes) in enumerate(sh):
        shape_tab[i, :2 + len(sizes)] = (K, len(sizes), *sizes)
    idx = np.array([(si, rows, *var, *KNOBS[k]) for si in range(len(sh)) for rows in ROWS for var, ks in VARIANTS for k in ks], dtype=np.int32)
    ans = evaluate(lib, nat, shape_tab, idx)
    assert np.abs(ans).max() < 2 ** 31
    path = os.path.join(HERE, "gemv_host_queries.npz")
    # (one array row per column of the table: that is what compresses)
    np.savez_compressed(path, shapes=shape_tab, queries=np.ascontiguousarray(idx.T), answers=np.ascontiguousarray(ans.T.astype(np.int32)))
    print(f"{nat.lib_path()}: {len(sh)} shapes, {len(idx)} rows, {os.path.getsize(path)} bytes; launch-shape errors recorded: {int((ans[:, 0] != 0).sum())}")


if __name__ == "__main__":
    main()
