"""Source-level regression pins (CPU).

Round 2's wrong tracking sums came from an inline-asm v_mad_i32_i24: an
INLINEASM statement carries no implicit EXEC operand, so machine passes may
move a non-volatile asm across the exec-mask writes of divergent branches,
where it writes lanes a branch had masked off (profiles/r3/mad24_hazard_repro_r3.log,
DESIGN.md section 3).  Every inline asm in the device sources must be volatile.
The repro form (TRACK_ASM_MAD) and the other measured-out tracking switches
(TRACK_SLOTS > 1 with its inline-asm slot read, TRACK_DMA_AUX, GNSSCORR_TRACK_V1,
TRACK_LOAD4) were removed in round 6; git history keeps them.
So does it keep the IQ half of osg_track_kernel, which osg_stream_kernel had replaced
on every product path, with its four environment switches, and the stream kernel's
seven compile-time switches that sat at their measured values and are constants now
(the names: `gone` below; none is part of a surviving identifier --
GNSSCORR_TRACK_XPF and GNSSCORR_TRACK_BALANCE stay).
The acquisition side followed: the fp32 engine's (acq32.hip, then part of acq.hip)
phase-ablation mask (ACQ_SKIP), cache-policy sweep (ACQ_LOAD_AUX), plane stride (ACQ_PLANE) and load-group (ACQ_LDGROUP) switches,
the one-unit kernel's ACQ_STAMP hook (pinned with its parenthesis; ACQ_PSTAMP and
ACQ64_STAMP stay) and GNSSCORR_ACQ_PIPE, which alone reached the best-of-blocks form
of acq_corr_kernel; and acq64_gen.hip's generic-engine switches M4_COLS2_PLANE (the
complex exchange of m4_cols2), M4_COLS2_WPE, M4_ROWS2_WPE, M4_ROWS2_ROWS, MX_WAVES,
M4_CT, M4_T2 and M4_RT, constants now (kM4ColThreads, kM4T2 and kM4RowThreads do not
contain the old spellings; M4_CASE stays).
"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "gnss-sdr.ru_amd", "csrc")


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            yield f, open(os.path.join(CSRC, f)).read().split("\n")


def test_inline_asm_is_volatile():
    bad = []
    for f, lines in _sources():
        for i, line in enumerate(lines, 1):
            t = line.strip()
            if re.search(r"\basm\s*\(", t):
                bad.append(f"{f}:{i}: {t}")
    assert not bad, "non-volatile inline asm:\n" + "\n".join(bad)


def test_measured_out_switches_are_gone():
    gone = ("TRACK_ASM_MAD", "TRACK_SLOTS", "TRACK_DMA_AUX", "GNSSCORR_TRACK_V1", "TRACK_LOAD4",
            # sgt.hip's compile-time switches, each measured and lost
            "SGT_KC32", "SGT_WPE", "SGT_PREFIX", "SGT_KSUB", "SGT_CHIPS", "SGT_CHIP_GROUP",
            "SGT_CHIP_FMA", "SGT_CHIP_PF", "SGT_SCHED",
            # the IQ half of osg_track_kernel: its environment switches ...
            "GNSSCORR_TRACK_STAGE_IF", "GNSSCORR_TRACK_PIECES", "GNSSCORR_TRACK_STREAM",
            "GNSSCORR_TRACK_CPW",
            # ... and osg_stream_kernel's settled compile-time switches
            "TRACK_NODUMP_COPY", "TRACK_IV4", "TRACK_ALIGNED", "TRACK_X2LUT", "TRACK_STREAM_CH",
            "TRACK_STREAM_WAVES", "TRACK_PF",
            # acq32.hip: the one-unit kernel's ablation and sweep switches, its stamp hook
            # (with the parenthesis: ACQ_PSTAMP stays) and the route past the pipelined kernel
            "ACQ_SKIP", "ACQ_LOAD_AUX", "ACQ_PLANE", "ACQ_LDGROUP", "ACQ_STAMP(",
            "GNSSCORR_ACQ_PIPE",
            # acq64_gen.hip: the generic engine's settled compile-time switches
            "M4_COLS2_PLANE", "M4_COLS2_WPE", "M4_ROWS2_WPE", "M4_ROWS2_ROWS", "MX_WAVES",
            "M4_CT", "M4_T2", "M4_RT")
    for f, lines in _sources():
        text = "\n".join(lines)
        for g in gone:
            assert g not in text, (f, g)
