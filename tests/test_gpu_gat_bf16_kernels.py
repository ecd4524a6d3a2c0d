"""The bf16-gather twins of the nine sparse attention kernels on the device (include/mggcn.h: mggcn_gat*_bf16), bit for bit
and without a tolerance: every entry on bf16 images gives the bits of its _f32 twin on the exactly widened operands -- on
every (VEC, NT, U) variant, over F / F^T = kernel_graph_long (rows of 0 .. 4097 entries) and the 200 x 320 block, for the
_drop forms, on misaligned and on 8-byte-aligned images, in the model's halves / thirds layout, and on a row range passed as
a call of its own.  The images are made on the host (bf16_ref.bf16_bits) with -0.0 and bf16 denormals planted; no NaN
(payload propagation is not part of the contract).  An operand in a gathered role is the image (bf16 call) or its widening
(fp32 call); an operand in an own-row role is the fp32 tensor in both."""
import numpy as np
import pytest

import bf16_ref as b16
import gat_ref as ref
import gatdot_ref as dot
import gatv2_ref as v2
from test_gpu_gat import _dense, _u32

pytestmark = pytest.mark.gpu

SHAPES = v2.RECT_SHAPES + [(1, 41)]          # one shape per compiled variant, then the last layer of the flagship epoch
GRAPHS = ("longT", "rect")
SENTINEL = 123.0
SENTINEL16 = 0x42F6                          # bf16(123.0)
DROP = (1 << 31, 2.0, 0x1234567887654321, 7, 1000, 70000)       # p = 0.5: threshold, scale, seed, stream, dst0, src0
VARIANTS = ("gat", "gatv2", "gatdot")


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _image_bits(x):
    """the bf16 image of x with -0.0 and two bf16 denormals planted (rows that the graphs gather)"""
    bits = b16.bf16_bits(x).copy()
    rows, d = bits.shape
    bits[0, 0], bits[1, d // 2], bits[rows - 1, d - 1] = 0x8000, 0x0001, 0x807F
    bits[2, :] = np.where(np.arange(d) % 3 == 0, 0x8000, bits[2, :])
    return bits


class _image:
    """a device bf16 image of ``rows x d`` elements at leading dimension d + pad, its base ``offset`` ELEMENTS past a 16-byte
    aligned allocation; pre-filled with bf16(123.0).  The interface of test_gpu_gat._dense."""
    esize = 2

    def __init__(self, rows, d, offset=0, pad=0, bits=None):
        torch = _torch()
        self.rows, self.d, self.ld = rows, d, d + pad
        self.flat = torch.full((rows * self.ld + offset + 8,), SENTINEL16, dtype=torch.int16, device="cuda")
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat[offset:offset + rows * self.ld].view(rows, self.ld)[:, :d]
        if bits is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)))
        self.ptr = self.flat.data_ptr() + 2 * offset


class _part:
    """columns [part d, (part + 1) d) of a wider device buffer (the model's halves and thirds)"""

    def __init__(self, whole, d, part):
        self.whole, self.d, self.ld, self.part, self.flat = whole, d, whole.ld, part, whole.flat
        self.esize = getattr(whole, "esize", 4)
        self.ptr = whole.ptr + self.esize * d * part

    def numpy(self):
        return self.whole.numpy()[:, self.part * self.d:(self.part + 1) * self.d].copy()


def _gathered(image, rows, d, offset, pad, bits):
    """an operand in a gathered role: the image for the bf16 call, its exact widening, equally aligned in elements, for the
    fp32 call"""
    if image:
        return _image(rows, d, offset, pad, bits)
    return _dense(rows, d, offset, pad, b16.widen(bits))


def _rows(p, r0):
    """the pointer of an operand moved by r0 rows"""
    return p.ptr + getattr(p, "esize", 4) * r0 * p.ld


class _chain:
    """the operands of one variant's three sparse calls on one graph; run() makes the calls in order and returns
    {output: (the matrix, the whole allocation)} as host arrays.  ``image``: the bf16 entries on images, else the fp32
    entries on the widened operands; ``off``: {gathered operand: elements} moves that operand's base, ``pad``: every leading
    dimension is d + pad; ``packed``: the gathered Z operands are parts of one [rows x parts d] buffer (square graphs)."""

    def __init__(self, ctx, kind, name, K, dh, image, off=None, pad=0, drop=None, packed=False, spoil=None):
        self.ctx, self.kind, self.K, self.dh, self.image, self.drop = ctx, kind, K, dh, image, drop
        self.sfx = "bf16" if image else "f32"
        indptr, indices, n_src = ref.edge_graphs()[name]
        self.n, self.n_src, d = indptr.size - 1, n_src, K * dh
        n = self.n
        t_indptr, t_indices = ref.transpose_pattern(indptr, indices, n_src)
        self.ip, self.ix, self.tip, self.tix = _u32(indptr), _u32(indices), _u32(t_indptr), _u32(t_indices)
        off = off or {}
        o = lambda k: off.get(k, 0)
        gath = lambda rows, key, host: _gathered(image, rows, d, o(key), pad, self._spoil(spoil, key, _image_bits(host)))
        own = lambda rows, host: _dense(rows, d, 0, pad, host)
        if kind == "gat":
            Z, Z_dst, G, att = ref.tolerance_inputs(n, n_src, K, dh)
            self.att = _dense(2, d, 0, 0, att)
            self.Z_own, self.Zd_own, self.G_own = own(n_src, Z), own(n, Z_dst), own(n, G)
            self.Z_g, self.G_g = gath(n_src, "Z", Z), gath(n, "G", G)
        elif kind == "gatv2":
            Zs, Zd, G, att = v2.inputs(n, n_src, K, dh)
            self.att = _dense(1, d, 0, 0, att)
            self.G_own = own(n, G)
            self.G_g = gath(n, "G", G)
            if packed:
                assert n == n_src
                own2 = _dense(n, 2 * d, 0, 0, np.concatenate([Zs, Zd], axis=1))
                g2 = _gathered(image, n, 2 * d, 0, 0, np.concatenate([_image_bits(Zs), _image_bits(Zd)], axis=1))
                self.Zs_own, self.Zd_own, self.Zs_g, self.Zd_g = _part(own2, d, 0), _part(own2, d, 1), _part(g2, d, 0), _part(g2, d, 1)
            else:
                self.Zs_own, self.Zd_own = own(n_src, Zs), own(n, Zd)
                self.Zs_g, self.Zd_g = gath(n_src, "Zs", Zs), gath(n, "Zd", Zd)
        else:
            Zq, Zk, Zv, G = dot.inputs(n, n_src, K, dh)
            self.G_own = own(n, G)
            self.G_g = gath(n, "G", G)
            if packed:
                assert n == n_src
                own3 = _dense(n, 3 * d, 0, 0, np.concatenate([Zq, Zk, Zv], axis=1))
                g3 = _gathered(image, n, 3 * d, 0, 0, np.concatenate([_image_bits(M) for M in (Zq, Zk, Zv)], axis=1))
                self.Zq_own, self.Zk_own, self.Zv_own = (_part(own3, d, i) for i in range(3))
                self.Zq_g, self.Zk_g, self.Zv_g = (_part(g3, d, i) for i in range(3))
            else:
                self.Zq_own, self.Zk_own, self.Zv_own = own(n, Zq), own(n_src, Zk), own(n_src, Zv)
                self.Zq_g, self.Zk_g, self.Zv_g = gath(n, "Zq", Zq), gath(n_src, "Zk", Zk), gath(n_src, "Zv", Zv)
        self.pad, self.d = pad, d
        self.scale = float(dot.default_scale(dh))

    @staticmethod
    def _spoil(spoil, key, bits):
        if spoil == key:
            bits[5, 1] ^= 0x0040                     # the top mantissa bit of one element of a gathered row: still finite
        return bits

    def outputs(self):
        """fresh output operands, pre-filled with 123.0"""
        n, n_src, d, K, pad = self.n, self.n_src, self.d, self.K, self.pad
        wide = dict(gat=dict(out=n, G_Z=n_src), gatv2=dict(out=n, G_Zd=n, P=n, G_Zs=n_src),
                    gatdot=dict(out=n, G_Zq=n, G_Zk=n_src, G_Zv=n_src))[self.kind]
        small = dict(gat=dict(s_dst=n, s_src=n_src, lse=n, D=n, ds_dst=n, ds_src=n_src), gatv2=dict(lse=n, D=n),
                     gatdot=dict(lse=n, D=n))[self.kind]
        o = {k: _dense(rows, d, 0, pad) for k, rows in wide.items()}
        o.update({k: _dense(rows, K) for k, rows in small.items()})
        return o

    def _entry(self, call, drop=None):
        return getattr(self.ctx.lib, f"mggcn_{self.kind}_{call}{'_drop' if drop is not None else ''}_{self.sfx}")

    def forward(self, o, r0=0, r1=None, drop=None):
        st, K, dh, n_src = self.ctx.stream(0), self.K, self.dh, self.n_src
        r1 = self.n if r1 is None else r1
        head = (st, r1 - r0, n_src, self.ip.data_ptr() + 4 * r0, self.ix.data_ptr())
        extra = () if drop is None else (*drop[:4], drop[4] + r0, drop[5])
        if self.kind == "gat":
            self._entry("forward", drop)(*head, self.Z_g.ptr, self.Z_g.ld, o["s_dst"].ptr + 4 * r0 * K, o["s_src"].ptr, K, dh,
                                         ref.SLOPE, _rows(o["out"], r0), o["out"].ld, o["lse"].ptr + 4 * r0 * K, *extra)
        elif self.kind == "gatv2":
            self._entry("forward")(*head, self.Zs_g.ptr, self.Zs_g.ld, _rows(self.Zd_own, r0), self.Zd_own.ld, self.att.ptr, K, dh,
                                   ref.SLOPE, _rows(o["out"], r0), o["out"].ld, o["lse"].ptr + 4 * r0 * K)
        else:
            self._entry("forward")(*head, _rows(self.Zq_own, r0), self.Zq_own.ld, self.Zk_g.ptr, self.Zk_g.ld, self.Zv_g.ptr,
                                   self.Zv_g.ld, K, dh, self.scale, _rows(o["out"], r0), o["out"].ld, o["lse"].ptr + 4 * r0 * K)

    def backward_dst(self, o, src, r0=0, r1=None, drop=None):
        """``src``: the outputs that hold the forward's out and lse (and the scores)"""
        st, K, dh, n_src = self.ctx.stream(0), self.K, self.dh, self.n_src
        r1 = self.n if r1 is None else r1
        head = (st, r1 - r0, n_src, self.ip.data_ptr() + 4 * r0, self.ix.data_ptr())
        extra = () if drop is None else (*drop[:4], drop[4] + r0, drop[5])
        k0 = 4 * r0 * K
        G, out = self.G_own, src["out"]
        if self.kind == "gat":
            self._entry("backward_dst", drop)(*head, self.Z_g.ptr, self.Z_g.ld, src["s_dst"].ptr + k0, src["s_src"].ptr,
                                              src["lse"].ptr + k0, _rows(G, r0), G.ld, _rows(out, r0), out.ld, K, dh, ref.SLOPE,
                                              o["D"].ptr + k0, o["ds_dst"].ptr + k0, *extra)
        elif self.kind == "gatv2":
            self._entry("backward_dst")(*head, self.Zs_g.ptr, self.Zs_g.ld, _rows(self.Zd_own, r0), self.Zd_own.ld, self.att.ptr,
                                        src["lse"].ptr + k0, _rows(G, r0), G.ld, _rows(out, r0), out.ld, K, dh, ref.SLOPE,
                                        o["D"].ptr + k0, _rows(o["G_Zd"], r0), o["G_Zd"].ld, _rows(o["P"], r0), o["P"].ld)
        else:
            self._entry("backward_dst")(*head, _rows(self.Zq_own, r0), self.Zq_own.ld, self.Zk_g.ptr, self.Zk_g.ld, self.Zv_g.ptr,
                                        self.Zv_g.ld, src["lse"].ptr + k0, _rows(G, r0), G.ld, _rows(out, r0), out.ld, K, dh,
                                        self.scale, o["D"].ptr + k0, _rows(o["G_Zq"], r0), o["G_Zq"].ld)

    def backward_src(self, o, src, r0=0, r1=None, drop=None):
        """``src``: the outputs that hold lse and D (and the scores, ds_dst) of all destinations"""
        st, K, dh, n = self.ctx.stream(0), self.K, self.dh, self.n
        r1 = self.n_src if r1 is None else r1
        head = (st, r1 - r0, n, self.tip.data_ptr() + 4 * r0, self.tix.data_ptr())
        extra = () if drop is None else (*drop[:5], drop[5] + r0)
        k0 = 4 * r0 * K
        if self.kind == "gat":
            square = self.n == self.n_src
            self._entry("backward_src", drop)(*head, _rows(self.Z_own, r0), self.Z_own.ld, src["s_dst"].ptr, src["s_src"].ptr + k0,
                                              src["lse"].ptr, src["D"].ptr, self.G_g.ptr, self.G_g.ld, self.att.ptr,
                                              src["ds_dst"].ptr + k0 if square else None, K, dh, ref.SLOPE, o["ds_src"].ptr + k0,
                                              _rows(o["G_Z"], r0), o["G_Z"].ld, *extra)
        elif self.kind == "gatv2":
            self._entry("backward_src")(*head, _rows(self.Zs_own, r0), self.Zs_own.ld, self.Zd_g.ptr, self.Zd_g.ld, self.att.ptr,
                                        src["lse"].ptr, src["D"].ptr, self.G_g.ptr, self.G_g.ld, K, dh, ref.SLOPE,
                                        _rows(o["G_Zs"], r0), o["G_Zs"].ld)
        else:
            self._entry("backward_src")(*head, self.Zq_g.ptr, self.Zq_g.ld, _rows(self.Zk_own, r0), self.Zk_own.ld,
                                        _rows(self.Zv_own, r0), self.Zv_own.ld, src["lse"].ptr, src["D"].ptr, self.G_g.ptr,
                                        self.G_g.ld, K, dh, self.scale, _rows(o["G_Zk"], r0), o["G_Zk"].ld, _rows(o["G_Zv"], r0),
                                        o["G_Zv"].ld)

    def scores(self, o):
        if self.kind != "gat":
            return
        lib, st, K, dh = self.ctx.lib, self.ctx.stream(0), self.K, self.dh
        lib.mggcn_gat_scores_f32(st, self.Zd_own.ptr, self.Zd_own.ld, self.att.ptr, o["s_dst"].ptr, None, self.n, K, dh)
        lib.mggcn_gat_scores_f32(st, self.Z_own.ptr, self.Z_own.ld, self.att.ptr, None, o["s_src"].ptr, self.n_src, K, dh)

    def run(self):
        """the three calls, each twice into the same outputs; host copies of every output and its whole allocation"""
        _torch().cuda.synchronize()
        o = self.outputs()
        self.scores(o)
        for _ in range(2):
            self.forward(o, drop=self.drop)
            self.backward_dst(o, o, drop=self.drop)
            self.backward_src(o, o, drop=self.drop)
        self.ctx.sync()
        self.o = o
        return {k: (m.numpy(), m.flat.cpu().numpy().copy()) for k, m in o.items()}


def _assert_twins(got, want, what, check_values=True):
    assert got.keys() == want.keys()
    for k in got:
        for i, nm in enumerate((k, f"the whole allocation of {k}")):
            np.testing.assert_array_equal(_bits(got[k][i]), _bits(want[k][i]), err_msg=f"{what}: {nm}")
        if check_values:
            assert np.isfinite(got[k][0]).all() and np.abs(got[k][0]).max() > 0, (what, k)


def _pair(ctx, kind, name, K, dh, **kw):
    return _chain(ctx, kind, name, K, dh, True, **kw).run(), _chain(ctx, kind, name, K, dh, False, **kw).run()


def test_the_shapes_reach_every_variant(pkg):
    assert set(pkg._lib.GAT_BF16_ENTRIES) <= set(pkg._lib.PROTOTYPES) and len(pkg._lib.GAT_BF16_ENTRIES) == 12
    got = {ref.head_geometry_for(dh, dh % 4 == 0)[0] for _, dh in SHAPES}
    assert got == {(4, 1, 4), (4, 4, 1), (1, 1, 4), (1, 4, 2), (1, 16, 1)}
    bits = _image_bits(np.ones((8, 8), dtype=np.float32))
    w = b16.widen(bits)
    assert np.signbit(w[0, 0]) and w[0, 0] == 0 and 0 < w[1, 4] < 1.17e-38 and -1.17e-38 < w[7, 7] < 0      # -0.0 and two denormals
    assert not np.isnan(w).any()


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("K,dh", SHAPES)
@pytest.mark.parametrize("kind", VARIANTS)
def test_bf16_call_gives_the_bits_of_the_fp32_call_on_the_widened_operands(ctx, kind, name, K, dh):
    """forward, backward_dst and backward_src of one variant, each run twice: every output and its whole allocation
    (padding columns, the floats past the end) carry the fp32 twin's bits"""
    got, want = _pair(ctx, kind, name, K, dh)
    _assert_twins(got, want, (kind, name, K, dh))


@pytest.mark.parametrize("K,dh", [(4, 32), (6, 7)])
def test_drop_forms(ctx, K, dh):
    """the three _drop_bf16 entries at p = 0.5, dst0 = 1000, src0 = 70 000 against the _drop_f32 entries on the widened
    operands; the mask really drops (the outputs differ from the plain call's); threshold 0 gives the plain bf16 entry's bits"""
    got, want = _pair(ctx, "gat", "longT", K, dh, drop=DROP)
    _assert_twins(got, want, ("drop", K, dh))
    plain = _chain(ctx, "gat", "longT", K, dh, True).run()
    assert (_bits(got["out"][0]) != _bits(plain["out"][0])).any() and (_bits(got["G_Z"][0]) != _bits(plain["G_Z"][0])).any()
    np.testing.assert_array_equal(_bits(got["lse"][0]), _bits(plain["lse"][0]))            # the softmax takes every entry
    zero = _chain(ctx, "gat", "longT", K, dh, True, drop=(0, 1.0) + DROP[2:]).run()
    _assert_twins(zero, plain, ("threshold 0", K, dh))


MOVED = [("gat", "Z"), ("gat", "G"), ("gatv2", "Zs"), ("gatv2", "Zd"), ("gatv2", "G"), ("gatdot", "Zk"), ("gatdot", "Zv"),
         ("gatdot", "Zq"), ("gatdot", "G")]


@pytest.mark.parametrize("kind,which", MOVED)
def test_a_misaligned_image_takes_the_element_path_with_the_same_bits(ctx, kind, which):
    """(4, 32) with one gathered image alone one element (2 bytes) off and every leading dimension d + 3: both calls take the
    element path (the fp32 twin is one float off) and give the same bits, which agree with the aligned run as another order
    of the same sums"""
    got, want = _pair(ctx, kind, "longT", 4, 32, off={which: 1}, pad=3)
    _assert_twins(got, want, (kind, which))
    aligned = _chain(ctx, kind, "longT", 4, 32, True).run()
    for k in got:
        assert ref.relerr(got[k][0], aligned[k][0]) <= 1e-4, (kind, which, k)
    moved = [k for k in got if (_bits(got[k][0]) != _bits(aligned[k][0])).any()]
    print(f"[gat bf16] {kind} {which} one element off: outputs with other bits than the aligned run: {moved}")
    assert moved, (kind, which)          # the element path is told apart by its bits: what the 8-byte test below relies on


@pytest.mark.parametrize("kind,which", MOVED)
def test_an_8_byte_aligned_image_takes_the_float4_path(ctx, kind, which):
    """the image base 8 modulo 16 (four elements past the allocation), ld = d: the bits of the 16-byte-aligned run, which
    the element path does not give on this shape (the test above asserts that it differs)"""
    moved = _chain(ctx, kind, "longT", 4, 32, True, off={which: 4})
    got = moved.run()
    g = {"Z": "Z_g", "G": "G_g"}.get(which, which + "_g")
    assert getattr(moved, g).ptr % 16 == 8
    _assert_twins(got, _chain(ctx, kind, "longT", 4, 32, True).run(), (kind, which))
    _assert_twins(got, _chain(ctx, kind, "longT", 4, 32, False, off={which: 4}).run(), (kind, which, "fp32 twin"))


@pytest.mark.parametrize("K,dh", [(4, 32), (3, 7)])
@pytest.mark.parametrize("kind", ["gatv2", "gatdot"])
def test_the_models_layout_gives_the_bits_of_separate_buffers(ctx, kind, K, dh):
    """Zs | Zd as the halves of one [n x 2 out] image and Zq | Zk | Zv as the thirds of one [n x 3 out] image (and the fp32
    operands likewise): the bits of separate buffers, and of the fp32 twin in the same layout"""
    got, want = _pair(ctx, kind, "longT", K, dh, packed=True)
    _assert_twins(got, want, (kind, "packed", K, dh))
    _assert_twins(got, _chain(ctx, kind, "longT", K, dh, True).run(), (kind, "apart", K, dh))


@pytest.mark.parametrize("kind,call,name,K,dh", [("gat", "forward", "longT", 4, 32), ("gatv2", "backward_dst", "rect", 3, 7),
                                                 ("gatdot", "backward_src", "longT", 2, 65)])
def test_a_row_range_gives_the_whole_calls_rows(ctx, kind, call, name, K, dh):
    """rows [5, 13) as a bf16 call of their own on outputs pre-filled with 123.0: the range carries the whole call's bits
    and every other row keeps its 123.0"""
    c = _chain(ctx, kind, name, K, dh, True)
    whole = c.run()
    o = c.outputs()
    if call == "forward":
        for k in ("s_dst", "s_src"):
            o[k] = c.o[k]
        c.forward(o, 5, 13)
        mine = ("out", "lse")
    elif call == "backward_dst":
        c.backward_dst(o, c.o, 5, 13)
        mine = ("D", "G_Zd", "P")
    else:
        c.backward_src(o, c.o, 5, 13)
        mine = ("G_Zk", "G_Zv")
    ctx.sync()
    for k in mine:
        got = o[k].numpy()
        np.testing.assert_array_equal(_bits(got[5:13]), _bits(whole[k][0][5:13]), err_msg=k)
        assert (np.delete(got, np.arange(5, 13), axis=0) == SENTINEL).all(), k
        assert np.abs(got[5:13]).max() > 0


@pytest.mark.parametrize("kind,which", [("gat", "Z"), ("gat", "G"), ("gatv2", "Zd"), ("gatdot", "Zv")])
def test_spoiling_one_image_element_changes_the_output(ctx, kind, which):
    got = _chain(ctx, kind, "longT", 4, 32, True, spoil=which).run()
    clean = _chain(ctx, kind, "longT", 4, 32, True).run()
    assert any((_bits(got[k][0]) != _bits(clean[k][0])).any() for k in got), (kind, which)


def test_the_image_is_what_is_read(pkg, ctx):
    """ops level, device conversion: Z (v1), Zs (GATv2), Zk and Zv (dot) are converted with ops.convert_bf16 and then filled
    with NaN -- the forwards take no fp32 copy of them -- and still give the bits of the fp32 wrapper on the widened images"""
    torch = _torch()
    ops, dn = pkg.ops, pkg.dn_matrix
    K, dh = 4, 32
    d = K * dh
    indptr, indices, n_src = ref.edge_graphs()["longT"]
    n = indptr.size - 1
    F = pkg.csr_matrix(indptr.copy(), indices.copy(), np.ones(indices.size, dtype=np.float32), n_src)

    def image_of(M):
        img = ops.bf16_image(torch.empty((M.n(), M.m()), dtype=torch.bfloat16, device="cuda"))
        ops.convert_bf16(ctx, M, img.t)
        ctx.sync()
        wide = dn(M.n(), M.m())
        wide.t.copy_((img.t.view(torch.int16).to(torch.int32) << 16).view(torch.float32))
        np.testing.assert_array_equal(img.t.view(torch.int16).cpu().numpy().view(np.uint16), b16.bf16_bits(M.numpy()))
        M.t.fill_(float("nan"))
        torch.cuda.synchronize()
        return img, wide

    def same(a, b):
        ctx.sync()
        for x, y in zip(a, b):
            np.testing.assert_array_equal(_bits(x.numpy()), _bits(y.numpy()))
            assert np.isfinite(x.numpy()).all() and np.abs(x.numpy()).max() > 0

    outs = lambda: (dn(n, d), dn(n, K))
    # v1: the scores come from the fp32 Z, before it is spoiled
    Z_h, _, _, att_h = ref.tolerance_inputs(n, n_src, K, dh)
    Z, att, s_dst, s_src = dn.from_numpy(Z_h), dn.from_numpy(att_h), dn(n, K), dn(n_src, K)
    ops.gat_scores(ctx, Z, att, s_dst, s_src, K)
    Z16, Zw = image_of(Z)
    a, b = outs(), outs()
    ops.gat_forward_bf16(ctx, F, Z16, s_dst, s_src, *a, K)
    ops.gat_forward(ctx, F, Zw, s_dst, s_src, *b, K)
    same(a, b)
    # GATv2
    Zs_h, Zd_h, _, att_h = v2.inputs(n, n_src, K, dh)
    Zs, Zd, att = dn.from_numpy(Zs_h), dn.from_numpy(Zd_h), dn.from_numpy(att_h)
    Zs16, Zsw = image_of(Zs)
    a, b = outs(), outs()
    ops.gatv2_forward_bf16(ctx, F, Zs16, Zd, att, *a, K)
    ops.gatv2_forward(ctx, F, Zsw, Zd, att, *b, K)
    same(a, b)
    # dot
    Zq_h, Zk_h, Zv_h, _ = dot.inputs(n, n_src, K, dh)
    Zq, Zk, Zv = dn.from_numpy(Zq_h), dn.from_numpy(Zk_h), dn.from_numpy(Zv_h)
    (Zk16, Zkw), (Zv16, Zvw) = image_of(Zk), image_of(Zv)
    a, b = outs(), outs()
    ops.gatdot_forward_bf16(ctx, F, Zq, Zk16, Zv16, *a, K)
    ops.gatdot_forward(ctx, F, Zq, Zkw, Zvw, *b, K)
    same(a, b)
    # the wrappers refuse an fp32 matrix where an image belongs, and the reverse, before the library
    with pytest.raises(ValueError, match="bf16 image"):
        ops.gat_forward_bf16(ctx, F, Zw, s_dst, s_src, *a, K)
    with pytest.raises(ValueError, match="bf16 image"):
        ops.gat_forward(ctx, F, Z16, s_dst, s_src, *a, K)
    ctx.sync()


@pytest.mark.parametrize("kind", VARIANTS)
def test_no_rows_launches_nothing(ctx, kind):
    """n_rows == 0 with null operands: nothing is launched, nothing is written"""
    lib, st = ctx.lib, ctx.stream(0)
    A, B = _dense(4, 16), _dense(4, 16)
    _torch().cuda.synchronize()
    S = ref.SLOPE
    if kind == "gat":
        lib.mggcn_gat_forward_bf16(st, 0, 7, None, None, None, 16, None, None, 4, 4, S, A.ptr, 16, None)
        lib.mggcn_gat_backward_dst_bf16(st, 0, 7, None, None, None, 16, None, None, None, None, 16, None, 16, 4, 4, S, A.ptr, B.ptr)
        lib.mggcn_gat_backward_src_bf16(st, 0, 7, None, None, None, 16, None, None, None, None, None, 16, None, None, 4, 4, S,
                                        A.ptr, B.ptr, 16)
        lib.mggcn_gat_forward_drop_bf16(st, 0, 7, None, None, None, 16, None, None, 4, 4, S, A.ptr, 16, None, *DROP)
    elif kind == "gatv2":
        lib.mggcn_gatv2_forward_bf16(st, 0, 7, None, None, None, 16, None, 16, None, 4, 4, S, A.ptr, 16, None)
        lib.mggcn_gatv2_backward_dst_bf16(st, 0, 7, None, None, None, 16, None, 16, None, None, None, 16, None, 16, 4, 4, S, None,
                                          A.ptr, 16, B.ptr, 16)
        lib.mggcn_gatv2_backward_src_bf16(st, 0, 7, None, None, None, 16, None, 16, None, None, None, None, 16, 4, 4, S, A.ptr, 16)
    else:
        lib.mggcn_gatdot_forward_bf16(st, 0, 7, None, None, None, 16, None, 16, None, 16, 4, 4, 0.5, A.ptr, 16, None)
        lib.mggcn_gatdot_backward_dst_bf16(st, 0, 7, None, None, None, 16, None, 16, None, 16, None, None, 16, None, 16, 4, 4, 0.5,
                                           None, A.ptr, 16)
        lib.mggcn_gatdot_backward_src_bf16(st, 0, 7, None, None, None, 16, None, 16, None, 16, None, None, None, 16, 4, 4, 0.5,
                                           A.ptr, 16, B.ptr, 16)
    ctx.sync()
    for t in (A.flat, B.flat):
        assert (t.cpu().numpy() == SENTINEL).all()
