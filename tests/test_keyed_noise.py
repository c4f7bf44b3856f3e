"""The rollout's keyed noise without a GPU (include/beso_noise.h, beso_amd/noise.py): the generator restated in numpy and pinned
to the published known answers, the header against the binding, and the argument errors of the three calls.  The restatement
here is the reference of tests/test_keyed_noise_gpu.py; the package holds none."""
import ctypes as C
import re

import numpy as np
import pytest

from beso_amd import _lib
from support import lib  # noqa: F401
from test_cabi import _ctypes_class, _header, _prototypes, declared_symbols, exported_symbols

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 of include/beso_noise.h on arrays: counter [..., 4] and key [..., 2] (broadcast against each other) ->
    the four words [..., 4], uint32.  uint64 arithmetic masked to 32 bits."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & U32 for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & U32 for i in range(2)]
    for r in range(10):
        if r:
            k = [(k[0] + np.uint64(W0)) & U32, (k[1] + np.uint64(W1)) & U32]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & U32]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def keyed_words(keys, episodes, steps, purpose, S, E):
    """beso_noise_words: [S, N, E] uint32 from keys [N] (Python ints below 2^64) and episodes / steps [N]."""
    N = len(keys)
    key = np.array([[k & 0xFFFFFFFF, k >> 32] for k in keys], dtype=np.uint64).reshape(1, N, 1, 2)
    q = (E + 3) // 4
    counter = np.zeros((S, N, q, 4), dtype=np.uint64)
    counter[..., 0] = np.arange(q).reshape(1, 1, q)
    counter[..., 1] = np.arange(S).reshape(S, 1, 1)
    counter[..., 2] = np.asarray(steps, dtype=np.uint64).reshape(1, N, 1)
    counter[..., 3] = ((np.asarray(episodes, dtype=np.uint64).reshape(1, N, 1) << np.uint64(4)) & U32) | np.uint64(purpose)
    return philox4x32_10(counter, key).reshape(S, N, 4 * q)[..., :E]


def normals_from_words(words, dtype=np.float64):
    """The Box-Muller expression of include/beso_noise.h on words [..., 4 q] evaluated in `dtype` -> [..., 4 q]."""
    w = np.asarray(words).reshape(words.shape[:-1] + (-1, 2, 2)).astype(np.uint64)
    two24 = dtype(2.0 ** -24)
    u = ((w[..., 0] >> np.uint64(8)) + np.uint64(1)).astype(dtype) * two24
    v = (w[..., 1] >> np.uint64(8)).astype(dtype) * two24
    r = np.sqrt(dtype(-2.0) * np.log(u))
    t = dtype(np.float32(6.2831855)) * v
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=-1).reshape(words.shape)


def keyed_normals(keys, episodes, steps, purpose, S, E, dtype=np.float64):
    q = (E + 3) // 4
    return normals_from_words(keyed_words(keys, episodes, steps, purpose, S, 4 * q), dtype)[..., :E]


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_restatement_gives_the_published_known_answers(counter, key, want):
    """Random123's kat_vectors for philox4x32_10: zero counter and key, all ones, and the digits of pi."""
    got = philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert [int(v) for v in got] == list(want)


def test_keyed_words_place_the_inputs_in_the_counter_and_the_key():
    """One block by hand: element 9 of slab 2, step 5, episode 3, purpose 1 under a key with a high word is word 1 of the block
    (9 / 4, 2, 5, 3 << 4 | 1); the value depends on nothing else -- not on N, not on the row."""
    key = (7 << 32) | 11
    want = philox4x32_10(np.array([2, 2, 5, 0x31], dtype=np.uint64), np.array([11, 7], dtype=np.uint64))[1]
    a = keyed_words([1, key], [0, 3], [9, 5], 1, 3, 10)
    b = keyed_words([key, 5, 6, 7], [3, 1, 1, 1], [5, 0, 0, 0], 1, 4, 13)
    assert int(a[2, 1, 9]) == int(b[2, 0, 9]) == int(want)
    assert np.array_equal(a[:, 1, :], b[:3, 0, :10])


def test_normals_are_finite_at_the_ends_of_the_uniforms():
    """The logarithm's argument is in (0, 1]: all-zero words give u = 2^-24 (the largest radius, sqrt(48 ln 2)), all-one words
    u = 1 (radius 0); no word gives a non-finite value."""
    z = normals_from_words(np.array([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF]], dtype=np.uint32))
    assert np.isfinite(z).all()
    assert abs(z[0, 0] - np.sqrt(48 * np.log(2))) < 1e-12 and z[0, 1] == 0 and z[0, 2] == 0 and z[0, 3] == 0


# ------------------------------------------------------------------------------------------------ the C ABI
def test_noise_header_matches_its_signature_table(lib):
    """include/beso_noise.h against _lib.NOISE_SIGNATURES with test_cabi.py's prototype parser: the same four functions in the
    header's order, per function the argument count, the class of every argument and the return type; the library exports
    exactly these; the enum and the limit agree with the binding's tables; libbeso_hip.so exports none of them."""
    protos, sigs = _prototypes("beso_noise.h"), _lib.NOISE_SIGNATURES
    assert sorted(protos) == sorted(sigs) == declared_symbols("beso_noise.h") and len(protos) == 4
    assert list(protos) == list(sigs) == list(_lib.NOISE_EXPORTS), "the table keeps the header's order"
    for fn, (ret, args) in protos.items():
        restype, argtypes = sigs[fn]
        assert len(argtypes) == len(args), f"{fn}: the header declares {len(args)} arguments, the table {len(argtypes)}"
        for i, (want, have) in enumerate(zip(args, argtypes)):
            assert _ctypes_class(have) == want, f"{fn}: argument {i} is {have!r} in the table, {want!r} in the header"
        assert _ctypes_class(restype) == ret, fn
    assert exported_symbols(_lib.NOISE_LIB_PATH) == sorted(protos)
    bound = _lib.load_noise()
    for fn in protos:
        assert len(getattr(bound, fn).argtypes) == len(sigs[fn][1])
    text = _header("beso_noise.h", keep_preprocessor=True)
    consts = {k: int(v) for k, v in re.findall(r"\b(BESO_NOISE_[A-Z_]+)\s*=?\s*(\d+)", text)}
    assert consts == {"BESO_NOISE_XT": _lib.NOISE_PURPOSES["x_t"], "BESO_NOISE_CANDIDATE": _lib.NOISE_PURPOSES["candidate"],
                      "BESO_NOISE_STEP": _lib.NOISE_PURPOSES["step"], "BESO_NOISE_MAX_PURPOSE": _lib.NOISE_LIMITS["max_purpose"]}
    have = exported_symbols(_lib.LIB_PATH)
    assert have == declared_symbols() == sorted(_lib.EXPORTS) and not set(have) & set(_lib.NOISE_EXPORTS)


def test_noise_argument_errors_are_named_before_anything_is_enqueued(lib):
    """Shapes below 1, arrays past the int range, an unknown purpose, NULL and misaligned pointers, a non-finite scale, a buffer
    without its count (and the reverse) and counters written over the counters read come back as a status with a message that
    names the function; a refused call touches no device (this test has none)."""
    nz = _lib.load_noise()
    one = 0x1000
    msg = lambda: nz.beso_noise_last_error().decode()                      # noqa: E731

    def plain(fn, **k):
        a = dict(keys=one, episodes=one, steps=one, N=3, purpose=0, S=2, E=7, out=one)
        a.update(k)
        head = [a[n] for n in ("keys", "episodes", "steps", "N", "purpose", "S", "E")]
        if fn == "beso_noise_normal":
            head.append(a.get("scale", 1.0))
        return getattr(nz, fn)(*head, a["out"], None)

    for fn in ("beso_noise_words", "beso_noise_normal"):
        for name in ("N", "S", "E"):
            assert plain(fn, **{name: 0}) == _lib.ERR_BAD_SHAPE and f"{name} = 0" in msg() and fn in msg(), (fn, name)
        assert plain(fn, N=1 << 11, S=1 << 10, E=1 << 10) == _lib.ERR_BAD_SHAPE and "int range" in msg()
        assert plain(fn, purpose=16) == _lib.ERR_BAD_ARG and "purpose = 16" in msg()
        assert plain(fn, purpose=-1) == _lib.ERR_BAD_ARG
        for name in ("keys", "episodes", "steps", "out"):
            assert plain(fn, **{name: None}) == _lib.ERR_BAD_ARG and "NULL pointer" in msg(), (fn, name)
            assert plain(fn, **{name: one + 2}) == _lib.ERR_BAD_ARG and "aligned" in msg(), (fn, name)
        assert plain(fn, keys=one + 4) == _lib.ERR_BAD_ARG and "aligned" in msg()
    for bad in (float("nan"), float("inf")):
        assert plain("beso_noise_normal", scale=bad) == _lib.ERR_BAD_ARG and "scale" in msg()

    def rollout(**k):
        a = dict(keys=one, reset=one, episodes_in=one, steps_in=2 * one, episodes_out=3 * one, steps_out=4 * one, N=5, act_dim=2,
                 K=3, n_steps=4, step_elems=18, x_t=one, cand=one, step_noise=one)
        a.update(k)
        return nz.beso_noise_rollout(*[a[n] for n in (
            "keys", "reset", "episodes_in", "steps_in", "episodes_out", "steps_out", "N", "act_dim", "K", "n_steps", "step_elems",
            "x_t", "cand", "step_noise")], None)

    assert rollout(N=0) == _lib.ERR_BAD_SHAPE and "N = 0" in msg() and "beso_noise_rollout" in msg()
    assert rollout(act_dim=0) == _lib.ERR_BAD_SHAPE and rollout(K=-1) == _lib.ERR_BAD_SHAPE and rollout(n_steps=-1) == _lib.ERR_BAD_SHAPE
    assert rollout(step_elems=0) == _lib.ERR_BAD_SHAPE and "step_elems = 0" in msg()
    assert rollout(N=1 << 20, n_steps=1 << 6, step_elems=1 << 6) == _lib.ERR_BAD_SHAPE and "int range" in msg()
    for name in ("keys", "episodes_in", "steps_in", "episodes_out", "steps_out", "x_t"):
        assert rollout(**{name: None}) == _lib.ERR_BAD_ARG and "NULL pointer" in msg(), name
    assert rollout(cand=None) == _lib.ERR_BAD_ARG and "cand" in msg()
    assert rollout(K=0) == _lib.ERR_BAD_ARG and "cand" in msg()
    assert rollout(step_noise=None) == _lib.ERR_BAD_ARG and "step_noise" in msg()
    assert rollout(n_steps=0) == _lib.ERR_BAD_ARG and "step_noise" in msg()
    assert rollout(x_t=one + 1) == _lib.ERR_BAD_ARG and "aligned" in msg()
    assert rollout(episodes_out=one) == _lib.ERR_BAD_ARG and "overlap" in msg()          # in place
    assert rollout(steps_out=2 * one + 8) == _lib.ERR_BAD_ARG and "overlap" in msg()     # 5 counters = 20 bytes
    assert rollout(steps_out=3 * one) == _lib.ERR_BAD_ARG and "overlap" in msg()         # both outputs in one array


def test_status_check_raises_value_errors_with_the_librarys_message(lib):
    nz = _lib.load_noise()
    status = nz.beso_noise_words(None, None, None, 1, 0, 1, 1, None, None)
    with pytest.raises(ValueError, match="beso_noise: words: beso_noise_words: a NULL pointer"):
        _lib.check_noise_status(status, "words")
    _lib.check_noise_status(_lib.OK, "nothing")


# ------------------------------------------------------------------------------------------------ the Python layer, no device
def test_seed_arguments_are_checked_on_the_host():
    from beso_amd.noise import check_seeds
    assert check_seeds(5, [0, 1, 2]) == [5, 6, 7], "an int is the seed of environment 0; environment i takes seed + i"
    assert check_seeds(2 ** 64 - 1, [0, 4]) == [2 ** 64 - 1, 3], "modulo 2^64"
    assert check_seeds([1, 2 ** 40, 2 ** 64 - 1], [4, 0, 2]) == [1, 2 ** 40, 2 ** 64 - 1]
    assert check_seeds(np.array([3, 4]), [0, 1]) == [3, 4]
    for bad in ([1, 2], [1, 2, -1], [1, 2, 2 ** 64], [1, 2, 3.5], [True, 1, 2], "abc", -1, 2 ** 64, 1.0, None):
        with pytest.raises(ValueError):
            check_seeds(bad, [0, 1, 2])


def test_predraw_noise_draws_what_it_drew_without_a_keyed_context():
    """No keyed context: predraw_noise makes the global generator's draws in the loop's order and number, zeros where a step
    draws nothing -- the expression it has always been; a given `noise=` of the right shape is returned as it is, untouched, and
    draws nothing."""
    import torch
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    sig = np.array([1.0, 0.5, 0.1, 0.0], dtype=np.float32)
    action = torch.zeros(2, 3, 4)
    for sampler, drawn in (("euler_ancestral", 2), ("dpm_2_ancestral", 2), ("dpmpp_2s_ancestral", 3)):
        torch.manual_seed(3)
        got = ks.predraw_noise(sampler, sig, action, 1.0)
        torch.manual_seed(3)
        want = torch.zeros(3, 2, 3, 4)
        for i in range(drawn):
            want[i] = torch.randn_like(action)
        assert torch.equal(got, want), sampler
        given = torch.full((3, 2, 3, 4), 7.0)
        torch.manual_seed(3)
        state = torch.get_rng_state()
        assert ks.predraw_noise(sampler, sig, action, 1.0, noise=given) is given
        assert torch.equal(torch.get_rng_state(), state)
    with pytest.raises(ValueError, match="noise"):
        ks.predraw_noise("euler_ancestral", sig, action, 1.0, noise=torch.zeros(2, 2, 3, 4))
