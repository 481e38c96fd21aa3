"""Host-side checks of the stream-batch C-ABI (stgcn_rt_streams, include/stgcn_amd.h), no GPU: the ctypes
descriptors have the C compiler's layout, bad descriptors are refused before any launch, and the addition left
the ABI version where it was."""
from test_cpu_host import _c_layout


def test_rt_streams_descriptor_layout(pkg, tmp_path):
    L = pkg._lib
    got, expect = _c_layout(tmp_path, {"stgcn_rt_streams_layer": L.RtStreamsLayer,
                                       "stgcn_rt_streams_desc": L.RtStreamsDesc})
    assert got == expect


def test_rt_streams_refuses_bad_descriptors(pkg):
    L = pkg._lib
    lib = L.load_library()
    assert lib.stgcn_rt_streams(None, None) == 1
    assert lib.stgcn_rt_streams(L.RtStreamsDesc(), None) == 1     # all null
    # every pointer and shape valid except B (the fake non-null pointers are never dereferenced on the host)
    d = L.RtStreamsDesc(V=25, L=1, C0=8, K=4, B=0, x=64, active=64, ln_w=64, ln_b=64, w_in=64, b_in=64, w_out=64,
                        b_out=64, out=64)
    y = d.layers[0]
    y.Cin, y.Cout, y.P, y.fifo_size, y.S, y.res_mode = 8, 8, 3, 9, 1, 1
    y.A = y.wp = y.bias2d = y.ln_w = y.ln_b = y.fifo = y.acc = y.idx = 64
    assert lib.stgcn_rt_streams(d, None) == 1                     # B = 0
    d.B, d.V = 4, 33
    assert lib.stgcn_rt_streams(d, None) == 1                     # V > 32
    d.V, y.Cout = 25, 6
    assert lib.stgcn_rt_streams(d, None) == 1                     # C % 4
    y.Cout, y.res_mode = 16, 1
    assert lib.stgcn_rt_streams(d, None) == 1                     # identity residual across a width change
    y.res_mode = 2
    assert lib.stgcn_rt_streams(d, None) == 1                     # res_mode 2 without the packed residual weight
    assert lib.stgcn_rt_streams_pack_elems(64, 64) == 2 * 4 * 512
    assert lib.stgcn_rt_streams_pack_elems(8, 8) == 512           # one zero-padded tile, one k-step
    assert lib.stgcn_rt_streams_pack_elems(64, 6) == -1
    assert lib.stgcn_rt_streams_pack_weight(None, 3, 64, 64, None, None) == 1
    assert lib.stgcn_rt_streams_pack_weight(64, 4, 64, 64, 64, None) == 1   # more groups than partitions


def test_abi_version_unchanged(pkg):
    assert pkg._lib.load_library().stgcn_abi_version() == 7
