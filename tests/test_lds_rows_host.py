"""Index model of the lane-contiguous first transposition of the planar 32 x 32 and 64 x 64 tile kernels
(transpose_tile<.., ROWS>, csrc/xcorr_tile.hpp).  No GPU.

The tile is 32 rows of 64 lanes at a pitch of 68 dwords: row k holds element k of every lane's line.  A lane stores
element k with `ds_write_addtid_b32 offset:272 k` (address = M0 + offset + 4 lane, two blocks of 16 stores per phase)
and reads the 32 values it needs -- one element of 32 lines -- as 8 `ds_read_b128` from dword (lane & 31) 68 + 32 h,
h = lane >> 5 (64 x 64, second phase: h ^ 1, the other lane half's columns).

Checked here, for both sizes and both phases:
  * every (line, element) is written exactly once, the two store blocks meet at k = 15 | 16, and the constants of the
    model are the ones the header holds (pitch, the 16 offsets of a store block, tile size);
  * every lane reads the right (line, element) into the right register, and every written cell is read exactly once;
  * no lane group of the LDS touches a bank twice: the two 32-lane halves of the stores, the four 16-lane service groups
    of `ds_read_b128`, and the two 32-lane groups of the `ds_read_b64` form at pitch 66 (the form an instance would fall
    back to if the 16-byte destinations cost it registers);
  * the model itself is not blind: a pitch of 64 fails the bank check, a wrong half offset fails the data check."""
import os
import re

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "torchpiv_amd", "csrc", "xcorr_tile.hpp")
PITCH = 68            # dwords per tile row
PITCH_B64 = 66        # the 8-byte-read fallback
ROWS = 32
# the lane groups that one LDS cycle serves (64-dword-wide LDS; 16-byte reads: four non-contiguous groups of 16)
GROUPS_B128 = [
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64)),
]
GROUPS_32 = [list(range(0, 32)), list(range(32, 64))]


def store_blocks(pitch):
    """[(M0 offset in dwords, [16 instruction offsets in dwords])] of the two store blocks of a phase."""
    return [(16 * pitch * blk, [pitch * q for q in range(16)]) for blk in range(2)]


def store_addr(base, off, lane):
    return base + off + lane                        # add-TID: M0 + offset + 4 lane (in dwords here)


def read_base(lane, ws, phase, pitch, half=32, swap=True):
    h = lane >> 5
    if ws == 64 and phase == 2 and swap:
        h ^= 1
    return (lane & 31) * pitch + half * h


def expected(lane, r, ws, phase):
    """(line, element) that register r of the phase's 32 holds after the transposition."""
    if ws == 32:                                    # lane (w, i): element i of line r of its own window
        return (lane & ~31) + r, lane & 31
    h, j = lane >> 5, lane & 31
    if phase == 1:                                  # diagonal blocks: line (h, r), low position j
        return 32 * h + r, j
    return 32 * (h ^ 1) + r, 32 + j                 # off-diagonal blocks: the other half's lines, high position 32 + j


def run_model(ws, phase, pitch=PITCH, width=4, half=32, swap=True):
    """Simulates one plane-phase.  Returns the bank-conflict findings; asserts the data path."""
    mem, rows = {}, []
    for base, offs in store_blocks(pitch):
        for off in offs:
            k = (base + off) // pitch
            rows.append(k)
            for lane in range(64):
                a = store_addr(base, off, lane)
                assert a not in mem, ("written twice", ws, phase, k, lane)
                mem[a] = (lane, k + (32 if (ws == 64 and phase == 2) else 0))
    assert rows == list(range(ROWS)), rows
    assert rows[15] == 15 and rows[16] == 16        # the two blocks meet at 15 | 16
    assert len(mem) == ROWS * 64
    assert max(mem) < ROWS * pitch                  # inside the tile
    # store banks: (a / 4) mod 32 within each 32-lane half
    conflicts = []
    for base, offs in store_blocks(pitch):
        for off in offs:
            for g in GROUPS_32:
                banks = [store_addr(base, off, lane) % 32 for lane in g]
                if len(set(banks)) != len(banks):
                    conflicts.append(("store", off))
    seen = set()
    groups = GROUPS_B128 if width == 4 else GROUPS_32
    for n in range(32 // width):                    # one wave-instruction
        addr = {lane: read_base(lane, ws, phase, pitch, half, swap) + width * n for lane in range(64)}
        for lane, a in addr.items():
            assert a % width == 0, ("misaligned read", lane, a)
            for q in range(width):
                assert a + q in mem, ("reads a cell nobody wrote", ws, phase, lane, a + q)
                assert mem[a + q] == expected(lane, width * n + q, ws, phase), (ws, phase, lane, width * n + q)
                assert a + q not in seen
                seen.add(a + q)
        for g in groups:                            # 8- and 16-byte reads: bank = (a / 4) mod 64
            banks = [(addr[lane] + q) % 64 for lane in g for q in range(width)]
            if len(set(banks)) != len(banks):
                conflicts.append(("read", n, g[0]))
    assert seen == set(mem)
    return conflicts


CASES = [(32, 1), (64, 1), (64, 2)]      # 32 x 32 has one phase per plane, 64 x 64 two


@pytest.mark.parametrize("ws,phase", CASES)
def test_every_cell_once_right_lane_no_conflict(ws, phase):
    assert run_model(ws, phase) == []


@pytest.mark.parametrize("ws,phase", CASES)
def test_b64_fallback_is_conflict_free(ws, phase):
    assert run_model(ws, phase, pitch=PITCH_B64, width=2) == []


@pytest.mark.parametrize("ws,phase", CASES)
def test_model_catches_a_wrong_pitch(ws, phase):
    """Pitch 64: the data still lands where it should, but every lane's 16-byte read starts on the same four banks."""
    found = run_model(ws, phase, pitch=64)
    assert found and all(kind == "read" for kind, *_ in found)
    assert len(found) == 8 * 4                      # every service group of every read


def test_model_catches_a_wrong_half_offset():
    with pytest.raises(AssertionError):
        run_model(64, 1, half=16)
    with pytest.raises(AssertionError):
        run_model(32, 1, half=16)
    with pytest.raises(AssertionError):             # phase 2 reading the lane half's OWN columns
        run_model(64, 2, swap=False)


def test_header_holds_the_models_constants():
    src = open(HEADER).read()
    assert int(re.search(r"ROW_PITCH\s*=\s*(\d+)\s*;", src).group(1)) == PITCH
    offs = [int(m) for m in re.findall(r"ds_write_addtid_b32 %\d+ offset:(\d+)", src)]
    assert offs == [4 * PITCH * q for q in range(16)], offs         # one block of 16 stores, bytes
    assert re.search(r"ROW_FLOATS\s*=.*32\s*\*\s*ROW_PITCH", src)
    assert (np.array(offs) < 1 << 16).all()                         # the instruction's offset field
