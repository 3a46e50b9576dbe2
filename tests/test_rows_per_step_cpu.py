"""CPU-only checks of the rule that says how many rows (segments) a barrier step of the staged
gather stages: pb_lbl_rows_per_step(rowlds, rowlim, &pitch), the host side of stage_slots() in
pb_ext_args.h.  The kernel calls the same function, so its seams are pinned here without a GPU."""
import ctypes as C

import numpy as np

PAD = 256          # kStagePad
CAP = 2            # kStageRowsMax


def rule(rowlds, rowlim):
    from pyratbay_amd import _capi
    pitch = C.c_int(-1)
    rows = _capi.call('pb_lbl_rows_per_step', int(rowlds), int(rowlim), C.byref(pitch))
    return rows, pitch.value


def test_seams_at_the_benchmark_geometry():
    """rowlds = 1002 (rows of up to 1001 samples): four slots fit up to 373 samples, six up to 163."""
    assert rule(1002, 373)[0] == 2
    assert rule(1002, 374)[0] == 1
    assert rule(1002, 163)[0] == min(CAP, 3)
    assert rule(1002, 164)[0] == 2
    assert rule(1002, 1001)[0] == 1
    assert rule(1002, 1)[0] == CAP
    # the pitch of a slot: the row plus one pad, rounded down to even (255 zeros suffice: a visit
    # reads 256 positions of which one at least holds row data)
    assert rule(1002, 373)[1] == 372 + PAD
    assert rule(1002, 299)[1] == 298 + PAD
    assert rule(1002, 300)[1] == 300 + PAD
    # one row per step keeps the layout of two full rows
    assert rule(1002, 374)[1] == 1002 + PAD
    assert rule(1002, 1002) == (1, 1002 + PAD)
    # and the pitch pointer is optional
    from pyratbay_amd import _capi
    assert _capi.call('pb_lbl_rows_per_step', 1002, 373, None) == 2


def test_slots_fit_the_row_area_for_every_geometry():
    """For every rowlds in 2..1024 and every rowlim <= rowlds: the 2 R slots end inside the area
    that plan_gather() sizes for two full rows, the pitch is even (slots start 16-byte aligned),
    R = 1 whenever the row is as long as the buffer, and a DMA piece that runs up to 127 samples
    past the end of a row stays inside the pad that follows its slot."""
    worst_rows = 0
    for rowlds in range(2, 1025):
        area = PAD + 2 * (rowlds + PAD)
        assert rule(rowlds, rowlds)[0] == 1
        for rowlim in range(1, rowlds + 1):
            rows, pitch = rule(rowlds, rowlim)
            assert 1 <= rows <= CAP
            assert pitch % 2 == 0
            assert PAD + 2 * rows * pitch <= area, (rowlds, rowlim, rows, pitch)
            if rows > 1:
                assert pitch == (rowlim + PAD) & ~1
                # at least 255 zeros between the data of two slots
                assert pitch - rowlim >= PAD - 1
                # the last sample a piece can write, against the start of the next slot
                assert -(-rowlim // 128) * 128 <= pitch
                # one more row per step would not fit (or the cap holds it back)
                assert rows == CAP or PAD + 2 * (rows + 1) * pitch > area
            else:
                # even rowlds (all the planner produces): exactly the two-buffer layout
                assert pitch == (rowlds + PAD) & ~1
            worst_rows = max(worst_rows, rows)
    assert worst_rows == CAP


def test_binding_and_header_agree():
    import os
    import re
    from pyratbay_amd import _capi, lbl
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'pbhip.h')).read()
    for name in ('pb_lbl_rows_per_step', 'pb_lbl_last_rows_per_step'):
        assert re.search(r'\b%s\s*\(' % name, text)
        assert name in _capi.exported_names()
    assert hasattr(lbl.LBL, 'last_rows_per_step')
    assert np.dtype(np.int32).itemsize == C.sizeof(C.c_int)
