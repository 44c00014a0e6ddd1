"""The (cin, cout) shapes each matrix-core operand format serves are pinned: the size queries answer without a GPU.  A shape
that silently left a table would run on the exact-fp32 kernel, and every numerical test would still pass."""
import itertools
import os

CHANNELS = (8, 16, 32, 64, 128, 256, 512)
SERVED = {(32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 32), (128, 64), (128, 128), (128, 256), (256, 128),
          (256, 256), (512, 64), (512, 128)}
# entry, bytes per channel, served shapes
FORMATS = [("df3d_conv_packed_weight_bytes", 4, SERVED),
           ("df3d_conv_packed_weight_bytes3", 6, SERVED),
           ("df3d_conv_packed_weight_bytes_bf16", 2, SERVED - {(128, 32), (512, 64), (512, 128)})]


def test_served_shapes_are_pinned():
    import __graft_entry__ as ge
    ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build").build()
    from dualfusion import _lib
    K = 27
    for entry, bytes_per_channel, served in FORMATS:
        query = getattr(_lib.load(), entry)
        for cin, cout in itertools.product(CHANNELS, CHANNELS):
            want = bytes_per_channel * K * cin * cout if (cin, cout) in served else 0
            assert query(K, cin, cout) == want, (entry, cin, cout)
            assert query(0, cin, cout) == 0, (entry, cin, cout)
