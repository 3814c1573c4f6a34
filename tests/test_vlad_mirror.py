"""The definition of the NetVLAD pooling (tests/np_mirror_vlad.py), without a GPU: the exact and the fast form agree, vlad_exp lies within
2 ulp of exp, the definition IS NetVLAD (within one float32 ulp of a plain float64 evaluation of the Keras layer), the ghost form is the
first K rows of the (K+G)-cluster softmax, and the data of the GPU cases tells the definition's orders from the ones it is not."""
import math

import numpy as np
import pytest

import np_mirror_vlad as M
import vlad_cases as T


# ---------------------------------------------------------------------------------------------- 1: exact form == fast form
@pytest.mark.parametrize("N,C,K,G", [(1, 4, 1, 0), (70, 8, 3, 1), (65, 12, 2, 0)])
def test_exact_form_equals_fast_form(N, C, K, G):
    Wt, bias, centres = T.weights(C, K, G, seed=3)
    x = T.fmap(N, C, seed=3)
    e, f = M.vlad_exact(x, Wt, bias, centres), M.vlad(x, Wt, bias, centres)
    for key in ("s", "a", "V", "A", "U", "v"):
        assert M.same_bits(e[key], f[key]), (key, M.first_difference(e[key], f[key]))


@pytest.mark.parametrize("name", T.CRAFTED)
def test_crafted_cases_exact_equals_fast_and_do_what_they_are_for(name):
    x, Wt, bias, centres, f = T.crafted_case(name)
    e = M.vlad_exact(x, Wt, bias, centres)
    for key in ("s", "a", "V", "A", "U", "v"):
        assert M.same_bits(e[key], f[key]), (key, M.first_difference(e[key], f[key]))
    a, v, K, C = f["a"], f["v"], centres.shape[0], x.shape[1]
    assert np.isfinite(v).all()
    if name == "far_apart":
        assert (a[:, 1] == 1.0).all() and (a[:, [0, 2, 3]] == 0.0).all()           # more than 700 below the largest: exact zeros
        assert (f["s"].max(axis=1) - f["s"].min(axis=1) > 700).all()
    elif name == "all_equal":
        assert (a == 0.25).all()
    elif name == "zero_position":
        b = bias.astype(np.float64)
        want = M.softmax(b[None, :])[0]
        assert M.same_bits(a[0], want) and M.same_bits(a[69], want)
    elif name == "dead_cluster":
        assert (a[:, 2] == 0.0).all() and (f["A"][2] == 0.0) and (v.reshape(K, C)[2] == 0.0).all() and (v != 0).any()
    elif name == "zero_map":
        assert (v == 0.0).all() and not np.signbit(v).any()


# ---------------------------------------------------------------------------------------------- 2: vlad_exp against mpmath
def test_vlad_exp_within_2_ulp_of_exp():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.prec = 200
    rng = np.random.default_rng(11)
    args = [0.0, -0.0, -700.0]
    for base in (0.0, -700.0, -1.0, -0.5 * math.log(2), -math.log(2), -1.5 * math.log(2), -354.89, -699.5):
        t = base
        for _ in range(4):                                         # the neighbours below (and, under 0, above)
            t = math.nextafter(t, -math.inf)
            if t >= -700.0:
                args.append(t)
        t = base
        for _ in range(4):
            t = math.nextafter(t, math.inf)
            if t <= 0.0:
                args.append(t)
    args += list(-700.0 * rng.random(3000)) + list(-rng.random(1000)) + list(-1e-3 * rng.random(200)) + [-(2.0 ** -k) for k in range(1, 60)]
    args += [(k + 0.5) * -math.log(2) for k in range(0, 1009, 7)]       # next to the ties of rint
    args = np.array(args)
    assert ((args <= 0) & (args >= -700.0)).all() and 0.0 in args and -700.0 in args
    got = M.vlad_exp(args)
    assert got[0] == 1.0 and got[1] == 1.0
    worst, at = 0.0, None
    for t, g in zip(args.tolist(), got.tolist()):
        want = mpmath.exp(mpmath.mpf(t))
        ulp = math.ulp(float(want))
        err = float(abs(mpmath.mpf(g) - want) / ulp)
        if err > worst:
            worst, at = err, t
    print(f"vlad_exp: worst error {worst:.3f} ulp at t = {at!r} over {args.size} arguments")     # measured: 1.0 ulp and a bit
    assert worst <= 2.0, (worst, at)
    sub = args[:: max(1, args.size // 300)]
    assert all(M.vlad_exp_exact(float(t)) == float(g) for t, g in zip(sub, M.vlad_exp(sub)))
    assert (M.vlad_exp(np.array([math.nextafter(-700.0, -math.inf), -701.0, -1e300, -np.inf])) == 0.0).all()
    assert M.vlad_exp(np.array([-700.0]))[0] > 0 and np.isfinite(np.log2(M.vlad_exp(np.array([-700.0]))[0]))   # a normal number


# ---------------------------------------------------------------------------------------------- 3: the definition IS NetVLAD
@pytest.mark.parametrize("N,C,K,G", [(130, 256, 8, 2), (1410, 512, 16, 0), (65, 260, 16, 0)])
def test_definition_is_netvlad_within_one_float32_ulp(N, C, K, G):
    x, Wt, bias, centres, f = T.shape_case(N, C, K, G)
    ref = M.keras_layer_f64(x, Wt, bias, centres)
    v = f["v"].astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(v - ref) <= ulp).all(), float((np.abs(v - ref) / ulp).max())
    differ = int((f["v"] != ref.astype(np.float32)).sum())
    print(f"{N} x {C}, K = {K}, G = {G}: {differ} of {v.size} components differ from (float) of the plain float64 evaluation")


# ---------------------------------------------------------------------------------------------- 4: ghosts
def test_ghost_form_is_the_first_K_rows_of_the_whole_softmax():
    N, C, K, G = 64, 256, 8, 2
    x, Wt, bias, centres, f = T.shape_case(N, C, K, G)
    assert f["a"].shape == (N, K + G) and f["V"].shape == (K, C) and f["v"].shape == (K * C,)
    # every cluster a kept one: the same assignment, and the kept rows aggregate the same way -- ghosts only take weight away
    more = np.concatenate([centres, np.zeros((G, C), np.float32)])
    g = M.vlad(x, Wt, bias, more)
    assert M.same_bits(g["a"], f["a"]) and M.same_bits(g["V"][:K], f["V"]) and M.same_bits(g["A"][:K], f["A"])
    assert (f["a"][:, K:] > 0).all() and (f["a"][:, :K].sum(axis=1) < 1).all()
    # without the ghost rows the assignment is another one
    h = M.vlad(x, Wt[:K], bias[:K], centres)
    assert not M.same_bits(h["a"], f["a"][:, :K])


# ---------------------------------------------------------------------------------------------- 5: the data tells the orders apart
def test_gpu_case_data_tells_the_block_order_and_mul_add_from_their_neighbours():
    """Device == mirror proves the block-of-64 order and the unfused multiply-add only if other orders give other bits on the same
    data.  On the GPU case 130 x 256, K = 8 + 2 (three blocks): V of one plain chain over n, and V with fma in the aggregation, each
    differ from the definition's V in at least a quarter of the K x C values (measured: 0.72 and 0.27; half the map is zero after the
    ReLU, and a zero term rounds the same way fused or not)."""
    N, C, K, G = 130, 256, 8, 2
    x, Wt, bias, centres = T.fmap(N, C), *T.weights(C, K, G)
    a = M.softmax(M.scores(x, Wt, bias))
    V, A = M.aggregate(a, x, K)
    Vp, Ap = M.aggregate(a, x, K, block=1 << 30)
    Vf, Af = M.aggregate(a, x, K, fused=True)
    share_plain = float((V != Vp).mean())
    share_fused = float((V != Vf).mean())
    print(f"V differs from one plain chain in {share_plain:.3f} and from the fma form in {share_fused:.3f} of {V.size} values; "
          f"A from the plain chain in {float((A != Ap).mean()):.3f}")
    assert share_plain >= 0.25 and share_fused >= 0.25
    assert M.same_bits(A, Af)                                       # the sums of a have no product in them
