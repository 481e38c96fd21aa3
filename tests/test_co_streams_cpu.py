"""Host-side checks of the co-st-gcn stream-batch C-ABI (stgcn_co_streams*, include/stgcn_amd.h), no GPU: the ctypes
descriptors have the C compiler's layout, bad descriptors are refused before any launch, the split count does not
depend on B, and the new symbols are exported."""
import pytest

from test_cpu_host import _c_layout

FAKE = 64  # a non-null pointer the host never dereferences


def make_desc(L, B=4, V=25, C0=8, layers=((8, 8, 3, 1, 1),), dtype=0):
    """Every pointer and shape valid; layers: (Cin, Cout, Kt, S, res_mode)."""
    d = L.CoStreamsDesc(B=B, V=V, L=len(layers), C0=C0, K=4, dtype=dtype, x=FAKE, active=FAKE, ln_w=FAKE, ln_b=FAKE,
                        w_in=FAKE, b_in=FAKE, w_out=FAKE, b_out=FAKE, h0=FAKE, order=FAKE, out=FAKE)
    for i, (cin, cout, kt, s, res) in enumerate(layers):
        y = d.layers[i]
        y.Cin, y.Cout, y.P, y.Kt, y.S, y.res_mode = cin, cout, 3, kt, s, res
        for f in ("A", "wp", "bias2d", "wrp", "br", "ln1_w", "ln1_b", "ln2_w", "ln2_b", "lnr_w", "lnr_b", "wt", "bt",
                  "ring", "res_ring", "idx", "z_buf", "r_buf", "partial", "y"):
            setattr(y, f, FAKE)
    return d


def test_co_streams_descriptor_layout(pkg, tmp_path):
    L = pkg._lib
    got, expect = _c_layout(tmp_path, {"stgcn_co_streams_layer": L.CoStreamsLayer,
                                       "stgcn_co_streams_desc": L.CoStreamsDesc})
    assert got == expect


def test_co_streams_symbols_exported(pkg):
    lib = pkg._lib.load_library()
    for name in ("stgcn_co_streams_splits", "stgcn_co_streams_workspace", "stgcn_co_streams"):
        assert hasattr(lib, name) and name in pkg._lib.EXPORTS
    assert lib.stgcn_abi_version() == 7


def _all(lib, d):
    return lib.stgcn_co_streams(d, None), lib.stgcn_co_streams_splits(d, 0), lib.stgcn_co_streams_workspace(d, 0)


def test_co_streams_refuses_bad_descriptors(pkg):
    L = pkg._lib
    lib = L.load_library()
    assert lib.stgcn_co_streams(None, None) == 1
    assert lib.stgcn_co_streams_splits(None, 0) == -1 and lib.stgcn_co_streams_workspace(None, 0) == -1
    assert _all(lib, L.CoStreamsDesc()) == (1, -1, -1)                     # all null and zero
    good = make_desc(L)
    assert lib.stgcn_co_streams_splits(good, 0) >= 1 and lib.stgcn_co_streams_workspace(good, 0) > 0
    assert lib.stgcn_co_streams_splits(good, 1) == -1                      # no such layer
    assert _all(lib, make_desc(L, B=0)) == (1, -1, -1)                     # B < 1
    assert _all(lib, make_desc(L, V=33)) == (1, -1, -1)                    # V > 32
    assert _all(lib, make_desc(L, C0=6, layers=((6, 8, 3, 1, 2),))) == (1, -1, -1)   # C % 4
    assert _all(lib, make_desc(L, layers=((8, 260, 3, 1, 2),))) == (1, -1, -1)       # C > 256
    assert _all(lib, make_desc(L, layers=((8, 8, 4, 1, 1),))) == (1, -1, -1)         # even Kt
    assert _all(lib, make_desc(L, layers=((8, 8, 71, 1, 1),))) == (1, -1, -1)        # Kt > 69
    assert _all(lib, make_desc(L, layers=((8, 8, 3, 3, 1),))) == (1, -1, -1)         # stride 3
    assert _all(lib, make_desc(L, layers=((8, 16, 3, 1, 1),))) == (1, -1, -1)        # identity residual, 8 -> 16
    assert _all(lib, make_desc(L, layers=((16, 16, 3, 1, 1),))) == (1, -1, -1)       # layer 0 Cin != C0
    assert _all(lib, make_desc(L, dtype=2)) == (2, -1, -1)                 # dtype outside {0, 1}
    d = make_desc(L)
    d.layers[0].P = 4
    assert _all(lib, d) == (1, -1, -1)                                     # P > 3
    d = make_desc(L)
    d.L = 13
    assert _all(lib, d) == (1, -1, -1)                                     # more than 12 layers
    # null pointers: the shape queries still answer, the tick is refused
    for field in ("x", "active", "ln_w", "w_in", "w_out", "h0", "order", "out"):
        d = make_desc(L)
        setattr(d, field, None)
        assert lib.stgcn_co_streams(d, None) == 1, field
        assert lib.stgcn_co_streams_splits(d, 0) >= 1
    for field in ("A", "wp", "ln1_w", "ln1_b", "ln2_w", "ln2_b", "wt", "ring", "res_ring", "idx", "z_buf", "partial", "y"):
        d = make_desc(L)
        setattr(d.layers[0], field, None)
        assert lib.stgcn_co_streams(d, None) == 1, field
    d = make_desc(L, layers=((8, 16, 3, 2, 2),))
    d.layers[0].wrp = None
    assert lib.stgcn_co_streams(d, None) == 1                              # residual conv without its packed weight


@pytest.mark.parametrize("layer", [(64, 64, 9, 1, 1), (64, 128, 9, 2, 2), (256, 256, 69, 1, 1), (8, 8, 3, 1, 1)])
def test_co_streams_splits_do_not_depend_on_B(pkg, layer):
    L = pkg._lib
    lib = L.load_library()
    counts, per_stream = set(), set()
    for B in (1, 2, 8, 64, 256, 1000):
        d = make_desc(L, B=B, C0=layer[0], layers=(layer,))
        n = lib.stgcn_co_streams_splits(d, 0)
        counts.add(n)
        nb = lib.stgcn_co_streams_workspace(d, 0)
        assert nb == B * n * 25 * layer[1] * 4
        per_stream.add(nb // B)
    assert len(counts) == 1 and min(counts) >= 1 and len(per_stream) == 1
    d = make_desc(L, B=8, C0=layer[0], layers=(layer,))
    d.layers[0].splits = 7
    nks = (layer[2] * layer[1] + 15) // 16
    assert lib.stgcn_co_streams_splits(d, 0) == min(7, nks)                # a forced count holds (up to the k-steps)
