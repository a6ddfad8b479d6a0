"""GPU: the packed weight of the bf16-pieces 1x1 kernel (orp_conv1x1_bn_pieces_pack_weight) byte for byte against the split computed
on the host: v0 = v & 0xffff0000, r = v - v0, v1 = r & 0xffff0000, v2 = r - v1, the high 16 bits of each as three planes
[3][Cin/16][2][Cout][8].  (64, 96): an output-channel count the split DeformConv packer's own shape rule refuses; (128, 64): more
than one 64-channel block, so the order of the channel blocks matters."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _host_planes(w):
    """w [Cout][Cin] fp32 (numpy) -> uint16 [3][Cin/16][2][Cout][8]"""
    cout, cin = w.shape
    mask = np.uint32(0xffff0000)
    planes, r = [], w.astype(np.float32)
    for _ in range(3):
        piece = (r.view(np.uint32) & mask).view(np.float32)
        planes.append((piece.view(np.uint32) >> np.uint32(16)).astype(np.uint16))
        r = (r - piece).astype(np.float32)            # exact: the piece is the leading bits of r
    assert not r.any()                                # 8 + 8 + 8 bits: nothing is left
    return np.stack([p.reshape(cout, cin // 16, 2, 8).transpose(1, 2, 0, 3) for p in planes])


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 96), (128, 64)])
def test_packed_planes_byte_for_byte(cin, cout):
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(100 * cin + cout)
    w = torch.randn(cout, cin, generator=g)
    flat = w.view(-1)
    special = [1.0, -2.0, 2.0 ** -20, -2.0 ** 30, 0.5, 0.0, -0.0, 3.4028e38]      # exact powers of two, both zeros, near FLT_MAX
    idx = torch.randperm(flat.numel(), generator=g)[:4 * len(special)]
    for k, v in enumerate(special):
        flat[idx[k::len(special)]] = v
    nbytes = L.orp_conv1x1_bn_pieces_packed_bytes(cin, cout)
    assert nbytes == 6 * cin * cout
    wd = w.to(dev).contiguous()
    packed = torch.full((nbytes,), 0xa5, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.orp_conv1x1_bn_pieces_pack_weight(_lib.ptr(wd), cin, cout, _lib.ptr(packed), _lib.stream_of(wd))
    _lib.check(rc, "orp_conv1x1_bn_pieces_pack_weight")
    torch.cuda.synchronize()
    got = packed.cpu().numpy().view(np.uint16).reshape(3, cin // 16, 2, cout, 8)
    assert np.array_equal(got, _host_planes(w.numpy()))
