"""The exact refinement (csrc/xcorr_exact.hip) keeps hand-issued ds_read_b32 spans in flight: one span of NDW + 2 dwords
for the arg-max's neighbourhood, two spans of NDW + 1 behind one wait for the other cells.  The compiler's own wait counting
does not see inline asm, so tools/check_lds_inflight.py walks the unit's device assembly: no register of a read may be
touched before the wait that covers it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import check_lds_inflight as C  # noqa: E402


def test_two_spans_behind_one_wait_are_checked():
    """The pattern of read_span2: both spans' destinations stay in flight until the one wait."""
    bad = """
_ZkernelA:
	;;#ASMSTART
	ds_read_b32 v4, v1 offset:0
	;;#ASMEND
	;;#ASMSTART
	ds_read_b32 v5, v2 offset:0
	;;#ASMEND
	v_alignbyte_b32 v6, v5, v4, v3
	;;#ASMSTART
	s_waitcnt lgkmcnt(0)
	;;#ASMEND
	s_endpgm
"""
    good = """
_ZkernelB:
	;;#ASMSTART
	ds_read_b32 v4, v1 offset:0
	;;#ASMEND
	;;#ASMSTART
	ds_read_b32 v5, v2 offset:0
	;;#ASMEND
	v_alignbyte_b32 v6, v8, v7, v3
	;;#ASMSTART
	s_waitcnt lgkmcnt(0)
	;;#ASMEND
	v_alignbyte_b32 v6, v5, v4, v3
	s_endpgm
"""
    assert len(C.check(bad)[0]) == 1 and C.check(good) == ([], 2)


def test_exact_refinement_reads_are_not_touched_before_their_wait(capsys):
    assert C.main("xcorr_exact") == 0
    n = int(capsys.readouterr().out.split(":")[1].split()[0])
    assert n > 0                         # (the unit still issues its spans by hand: the walk saw them)
