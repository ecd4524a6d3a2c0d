"""The bf16 MLP link decoder without a GPU: the refusals of mlp_link_predictor(decoder_dtype=) and of the bf16 ops (each raises
before any device call), the exported symbols, and the sanity of tests/link_mlp_bf16_ref.py's rounding family."""
import numpy as np
import pytest

import link_mlp_bf16_ref as ref
import link_mlp_ref
import link_ref
from bf16_ref import round_bf16
from test_link_cpu import _model, _P, fake


class fake16(fake):
    """a 2-byte fake with a row pitch of its own"""
    pitch = None

    def element_size(self): return 2
    def stride(self, i): return (self.pitch or self.shape[1]) if i == 0 else 1


@pytest.mark.parametrize("dtype", ("fp16", "BF16", None, 16))
def test_unknown_decoder_dtype_is_refused(pkg, dtype):
    with pytest.raises(ValueError, match="decoder_dtype"):
        pkg.mlp_link_predictor(_model(pkg, d=32), _P(pkg), decoder_dtype=dtype)


@pytest.mark.parametrize("case,word", [("d", "embedding width"), ("hd", "hd"), ("pitch", "pitch"), ("base", "pitch"), ("fp32_H", "bf16"),
                                       ("image_len", "image"), ("image_align", "image"), ("image_f32", "image"), ("ld", "G must be"),
                                       ("overlap", "overlap"), ("n31", "below 2"), ("pack_d", "embedding width"), ("pack_on_W1", "overlap")])
def test_the_bf16_ops_refuse(pkg, case, word):
    ops, f = pkg.ops, lambda *s: fake(1 << 20, *s, floating=True)
    d, hd = (48, 64) if case == "d" else (32, 48) if case == "hd" else (32, 64)
    halves = ops.link_mlp_image_halves(d, hd) if d % 32 == 0 and hd % 32 == 0 else 8
    Hb = fake16(1 << 24, 10, d)
    Hb.pitch = d + 2 if case == "pitch" else None
    image = fake16(1 << 26, halves)
    if case == "base":
        Hb = fake16((1 << 24) + 4, 10, d)
    elif case == "fp32_H":
        Hb = fake(1 << 24, 10, d, floating=True)
    elif case == "image_len":
        image = fake16(1 << 26, halves - 8)
    elif case == "image_align":
        image = fake16((1 << 26) + 8, halves)
    elif case == "image_f32":
        image = fake(1 << 26, d, hd, floating=True)
    params = (image, fake(2 << 20, hd, floating=True), fake(3 << 20, hd, floating=True), fake(4 << 20, 1, floating=True))
    G = fake(5 << 20, 10, d + 4 if case == "ld" else d, floating=True)
    if case == "overlap":
        G = fake((1 << 24) + 64, 10, d, floating=True)
    with pytest.raises(ValueError, match=word):
        if case.startswith("pack"):
            W1 = f(48 if case == "pack_d" else 32, 64)
            ops.link_mlp_pack_bf16(None, W1, fake16((1 << 20) + 16 if case == "pack_on_W1" else 1 << 26, ops.link_mlp_image_halves(32, 64)))
        elif case == "n31":
            ops.link_mlp_loss_bf16(None, 1 << 31, 10, fake(64, 11), fake(512, 3), 3, Hb, params, G, True, 1.0)
        else:
            ops.link_mlp_loss_bf16(None, 10, 10, fake(64, 11), fake(512, 3), 3, Hb, params, G, True, 1.0)
    if case in ("pitch", "base", "fp32_H", "image_len", "image_align", "image_f32", "d", "hd"):
        with pytest.raises(ValueError, match=word):
            ops.link_mlp_pairs_bf16(None, Hb, params, pairs=(fake(64, 5), fake(128, 5), 5), out=fake(6 << 20, 5, floating=True))


def test_exports(pkg):
    lib = pkg._lib.load()
    for name in ("link_mlp_loss_bf16", "link_mlp_pairs_bf16", "link_mlp_pack_bf16", "link_mlp_image_halves"):
        assert hasattr(lib, "mggcn_" + name) and "mggcn_" + name in pkg._lib.PROTOTYPES and hasattr(pkg.ops, name)
    assert lib.mggcn_link_mlp_image_halves(96, 64) == pkg.ops.link_mlp_image_halves(96, 64) == 64 * (96 + 8) + 96 * (64 + 8)


def test_the_rounding_family_is_what_it_claims():
    n, d, hd, R = 70, 128, 128, 2
    indptr, indices = link_ref.pattern(n, 14)
    pairs = link_mlp_ref.pairs_of(indptr, indices, n, R, 3, 1)
    (us, vs), (H, params) = pairs[:2], ref.rounding_inputs(n, d, hd, 0, *pairs[:2])
    Hb = round_bf16(H)
    assert ((H.view(np.uint32) & 0xFFFF0000).view(np.float32) != Hb).any()                  # truncation is not the rounding
    exact = Hb[us].astype(np.float64) * Hb[vs]
    assert (round_bf16(exact.astype(np.float32)) != exact).mean() > 0.9                     # x needs its own rounding
    want, twin = (ref.loss_grad(H, params, *pairs, dt=dt) for dt in (np.float64, np.float32))
    z = ref.check(want, twin) or want["z"]
    assert ((z * 8192) % 2 == 1).all() and np.abs(z).max() < 2 ** 9                         # odd multiples of 2^-13: exact in fp32
    unrounded = (H[us].astype(np.float64) * H[vs]) @ params[0] + params[1]                  # a decoder that reads the fp32 operands
    assert np.abs(unrounded - z).max() > 5e-4 * np.abs(z).max()
