"""No-GPU checks of the snapshot / fork / return code (jitterbug_amd/csrc/jb_snapshot.hpp): the element functions the two device
kernels are made of, compiled for the host (tests/snapshot_harness.cpp) and compared with numpy restatements of the layout; the
refusals of the blob header; the NULL-handle answers of the new entry points; and one stand-alone sanitizer run of the host code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.build_harness import build_source

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "snapshot_harness.cpp")
ROOT_F, LEG_F, WORDS = 32, 6, 58


@pytest.fixture(scope="module")
def hs():
    lib = C.CDLL(build_source(SRC, "libjb_snapshot_host.so", ["-Wall", "-O2", "-fPIC", "-shared"]))
    vp = C.c_void_p
    lib.jbs_fork.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp]
    lib.jbs_fork.restype = None
    lib.jbs_return.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, vp, vp]
    lib.jbs_return.restype = None
    lib.jbs_make_header.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.jbs_make_header.restype = None
    lib.jbs_check_header.argtypes = [vp, C.c_longlong, C.c_int, C.c_char_p, C.c_int]
    lib.jbs_first_bad_index.argtypes = [vp, C.c_int, C.c_int]
    assert lib.jbs_words_per_env() == WORDS and lib.jbs_header_bytes() == 64
    return lib


def synth(n, seed):
    """a snapshot of n envs with random words, as its four blocks"""
    rng = np.random.default_rng(seed)
    def w(*shape):
        return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    return w(ROOT_F, n), w(LEG_F, n, 4), w(n), w(n)


def flat(blocks):
    return np.concatenate([b.reshape(-1) for b in blocks])


def gathered(blocks, s):
    root, leg, step, ep = blocks
    return root[:, s], leg[:, s, :], step[s], ep[s]


FORK_CASES = [
    # (label, n_dst, n_src, map)
    ("straight-copy", 37, 37, None),
    ("permutation", 37, 37, lambda n, m: (np.arange(n) * 7 + 3) % m),
    ("fan-out-2-to-128", 128, 2, lambda n, m: np.arange(n) // 64),
    ("fan-out-1-to-5", 5, 1, lambda n, m: np.zeros(n, int)),
    ("group-leaders", 256, 256, lambda n, m: 8 * (np.arange(n) // 8)),
    ("clamped", 9, 3, lambda n, m: np.array([-1, 3, 2, 0, m, -2 ** 31, 2 ** 31 - 1, 1, 0])),
    ("no-map-smaller-source-is-clamped", 9, 3, None),
]


@pytest.mark.parametrize("label,n_dst,n_src,mapf", FORK_CASES, ids=[c[0] for c in FORK_CASES])
@pytest.mark.parametrize("split", [False, True], ids=["flat-destination", "four-block-destination"])
def test_fork_word_gathers_every_block(hs, label, n_dst, n_src, mapf, split):
    src = synth(n_src, 1)
    m = None if mapf is None else np.ascontiguousarray(mapf(n_dst, n_src), dtype=np.int32)
    s = np.clip(np.arange(n_dst) if m is None else m.astype(np.int64), 0, n_src - 1)      # what the kernel promises: clamped into [0, n_src)
    want = gathered(src, s)
    src_flat = flat(src)
    if split:
        out = [np.full(b.shape, 0xDEADBEEF, dtype=np.uint32) for b in want]
        hs.jbs_fork(None, *[o.ctypes.data for o in out], n_dst, src_flat.ctypes.data, n_src, None if m is None else m.ctypes.data)
        for o, b in zip(out, want):
            assert np.array_equal(o, b)
    else:
        out = np.full(WORDS * n_dst, 0xDEADBEEF, dtype=np.uint32)
        hs.jbs_fork(out.ctypes.data, None, None, None, None, n_dst, src_flat.ctypes.data, n_src, None if m is None else m.ctypes.data)
        assert np.array_equal(out, flat(want))
    if label == "straight-copy" and not split:
        assert np.array_equal(out, src_flat)


def reference_return(r, d, gamma32):
    """the recurrence of jb_snapshot.hpp in numpy float32: acc = fma(g, r, acc); stop if done; g *= gamma - r here is exactly representable
    so that fp32 products and sums are exact and the comparison is for equality"""
    K, N = r.shape
    out, alive = np.zeros(N, np.float32), np.zeros(N, np.int32)
    for n in range(N):
        acc, g = np.float64(0), np.float32(1)
        k = 0
        while k < K:
            acc = np.float32(np.float64(g) * np.float64(r[k, n]) + np.float64(acc))      # one rounding: a fused multiply-add
            k += 1
            if d[k - 1, n]:
                break
            g = np.float32(g * gamma32)
        out[n], alive[n] = acc, k
    return out, alive


@pytest.mark.parametrize("gamma", [1.0, 0.9])
def test_return_recurrence_on_hand_made_arrays(hs, gamma):
    K, N = 6, 5
    r = (np.arange(K * N, dtype=np.float32).reshape(K, N) % 7 - 3) * np.float32(0.25)
    d = np.zeros((K, N), dtype=np.uint8)
    d[0, 0] = 1                    # done at step 0: only r[0] counts
    d[K - 1, 1] = 1                # done at the last step: all K count
    d[2, 3] = 1; d[4, 3] = 1       # done twice: what follows the FIRST belongs to another episode
    d[3, 4] = 1                    # env 2: never done
    out, alive = np.zeros(N, np.float32), np.zeros(N, np.int32)
    g32 = np.float32(gamma)
    hs.jbs_return(r.ctypes.data, d.ctypes.data, K, N, C.c_float(gamma), out.ctypes.data, alive.ctypes.data)
    assert list(alive) == [1, K, K, 3, 4]
    assert out[0] == r[0, 0]
    want, want_alive = reference_return(r, d, g32)
    assert np.array_equal(alive, want_alive)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    # against fp64 with the bound the GPU test uses: K * 2^-23 * sum gamma^k |r_k|
    for n in range(N):
        gk = np.float64(g32) ** np.arange(alive[n])
        exact = (gk * r[:alive[n], n].astype(np.float64)).sum()
        assert abs(float(out[n]) - exact) <= K * 2.0 ** -23 * (gk * np.abs(r[:alive[n], n])).sum()
    if gamma == 1.0:
        assert out[2] == r[:, 2].sum() and out[3] == r[:3, 3].sum()


def test_blob_header_and_map_checks(hs):
    n, task = 12, 4
    blob = np.zeros(64 + 232 * n, dtype=np.uint8)
    hs.jbs_make_header(blob.ctypes.data, n, task, 50, 1000)
    hd = blob[:64].view(np.int32)
    assert blob[:4].tobytes() == b"JBSN" and list(hd[1:8]) == [1, n, task, 50, 1000, ROOT_F, LEG_F] and not hd[8:].any()
    why = C.create_string_buffer(128)
    assert hs.jbs_check_header(blob.ctypes.data, blob.size, task, why, 128) == 0
    assert hs.jbs_check_header(blob.ctypes.data, blob.size - 232, task, why, 128) == 1 and b"size" in why.value      # truncated
    assert hs.jbs_check_header(blob.ctypes.data, blob.size + 1, task, why, 128) == 1
    assert hs.jbs_check_header(blob.ctypes.data, 63, task, why, 128) == 1
    assert hs.jbs_check_header(blob.ctypes.data, blob.size, task - 1, why, 128) == 1 and b"task" in why.value
    for word, msg in ((0, b"magic"), (1, b"version"), (6, b"field"), (7, b"field")):
        bad = blob.copy()
        bad[:64].view(np.int32)[word] += 1
        assert hs.jbs_check_header(bad.ctypes.data, bad.size, task, why, 128) == 1 and msg in why.value, word
    m = np.array([0, 11, 12, -1], dtype=np.int32)
    assert hs.jbs_first_bad_index(m.ctypes.data, 2, n) == -1
    assert hs.jbs_first_bad_index(m.ctypes.data, 4, n) == 2           # n_src itself is outside
    assert hs.jbs_first_bad_index(m.ctypes.data, 4, n + 1) == 3       # ... and so is -1


def test_new_entry_points_refuse_a_null_handle():
    from jitterbug_amd import _lib, build
    build.build()
    lib = _lib.load()
    for call in (lambda: lib.jb_snapshot_bytes(None), lambda: lib.jb_snapshot_host_bytes(None), lambda: lib.jb_snapshot_device(None, None),
                 lambda: lib.jb_restore_device(None, None, 1, None), lambda: lib.jb_snapshot(None, None), lambda: lib.jb_restore(None, None, 0, None),
                 lambda: lib.jb_score_tapes_device(None, 1, None, 1.0, None, None)):
        assert call() == -1 and b"NULL" in lib.jb_last_error()


def test_host_code_under_address_and_undefined_sanitizers():
    """The one sanitizer run of this code: a stand-alone program (its own main, tests/snapshot_harness.cpp -DJBS_MAIN) over the ragged,
    fan-out and clamped cases, on heap blocks of exactly the promised sizes."""
    # (the sanitizer runtimes are linked statically: the program is complete in itself, whatever else the process environment loads)
    exe = build_source(SRC, "snapshot_harness_san", ["-Wall", "-O1", "-g", "-DJBS_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = p.stdout.decode("utf-8", "replace")
    assert p.returncode == 0 and "all ok" in text and "MISMATCH" not in text and "runtime error" not in text, text
