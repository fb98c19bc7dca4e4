"""The layout-matrix shape of the lane kernels' GPU tests (k_codel, k_inbound, k_outbound).

Each kernel has four compiled walk sites: LM = 0 (contiguous chunks only), LM = 1 (lane-major
only), and LM = 2 with a block that goes lane-major and one that stays contiguous
(ChunkMap<false> through the shared walk).  One call of this shape under SG_LANE_MAJOR unset,
"0" and "1" reaches all four.

128 hosts, two blocks of 64: hosts 0-63 get 48 events each, host 64 gets 3,000, hosts 65 and
66 get 3 each, the rest none; E = 6,078.  By lane_major_launch and lane_major_block
(sg_codel.hip, sg_lanes.h; CHUNK_COST = 10), with CH the kernel's chunk (1,024 k_codel and
k_inbound, 896 k_outbound, 512 k_outbound keyed) and LK = CH / 64:

* unset launches LM = 2: E = 6,078 > 2 CH nb = 4,096 / 3,584 / 2,048 (nb = 2 blocks).
* block 0 (3,072 events > 2 CH, busiest host 48, 64 active, mean 48) goes lane-major:
  contiguous ceil(3,072 / CH) (10 + 48) = 174 / 232 / 348 against lane-major
  ceil(48 / LK) (10 + LK) = 3 x 26 = 78 / 4 x 24 = 96 / 6 x 18 = 108.
* block 1 (3,006 events, busiest host 3,000, 3 active, mean 1,002) stays contiguous:
  ceil(3,006 / CH) (10 + min(1,002, CH)) = 3 x 1,012 = 3,036 / 4 x 906 = 3,624 /
  6 x 522 = 3,132 against ceil(3,000 / LK) (10 + LK) = 188 x 26 = 4,888 / 215 x 24 = 5,160 /
  375 x 18 = 6,750.

Host 64 spans three to six contiguous chunks and 188 to 375 lane-major ones; hosts 65 and 66
sit behind it in the last chunk; hosts 67-127 have an empty range in every chunk.
"""
import numpy as np

H = 128
RING_CAP = 4096
LAYOUTS = ("", "0", "1")  # SG_LANE_MAJOR unset (per block), contiguous, lane-major


def host_column():
    """The events' hosts, grouped by ascending host."""
    n = np.zeros(H, np.int64)
    n[:64] = 48
    n[64] = 3000
    n[65:67] = 3
    return np.repeat(np.arange(H, dtype=np.uint32), n)


def set_layout(monkeypatch, layout):
    if layout:
        monkeypatch.setenv("SG_LANE_MAJOR", layout)
    else:
        monkeypatch.delenv("SG_LANE_MAJOR", raising=False)
