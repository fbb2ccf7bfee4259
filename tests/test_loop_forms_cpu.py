"""Which time-loop form pkc_rnn_fwd / pkc_rnn_bwd take for a layer (pkc_rnn_persist_form,
include/pkc.h: 1 the liGRU loops, 2 the grid-synchronised loops, 0 one launch per step) at the
BASELINE sequence configs' layer shapes, and where the rules fall back.  The function reads only
the argument struct and the environment (with no device it assumes 256 compute units), so the
dispatch rules are checked here without a GPU; tests/test_gpu_lstm_persist.py checks each loop
against the per-step launches on the GPU."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-kaldi-cgs_amd"))


def _args(cell, H, B, bidir=False, **kw):
    """An RnnArgs with non-null placeholder pointers (never dereferenced by the form query)."""
    from pkc import _lib as L
    a = L.RnnArgs()
    a.cell, a.T, a.B, a.H, a.bidir = cell, 40, B, H, int(bidir)
    p = C.c_void_p(4096)
    for f in ("wpre", "hs", "cs", "gates", "y", "dy", "dgates", "work", "ut"):
        setattr(a, f, p)
    for g in range(4):
        a.U[g] = p
    for k, v in kw.items():
        if k == "U_h":
            for g in range(4):
                a.U_h[g] = p if v else None
        elif isinstance(v, bool):
            setattr(a, k, p if v else None)
        else:
            setattr(a, k, v)
    return a


def _form(a):
    from pkc import _lib as L
    lib = L.lib()
    return lib.pkc_rnn_persist_form(C.byref(a), 0), lib.pkc_rnn_persist_form(C.byref(a), 1)


def test_c4_lstm_fp32_and_bf16_take_the_grid_loops():
    from pkc import _lib as L
    # C4: 4 x 1024 bidirectional, B = 16 (32 rows)
    assert _form(_args(L.CELL_LSTM, 1024, 16, True)) == (2, 2)
    assert _form(_args(L.CELL_LSTM, 1024, 16, True, step_bf16=1, hs_h=True, U_h=True,
                       ut_h=True, dgates_h=True)) == (2, 2)
    assert _form(_args(L.CELL_LSTM, 512, 12, False)) == (2, 2)
    assert _form(_args(L.CELL_LSTM, 768, 10, True)) == (2, 2)


def test_c5_quantised_h_loops():
    from pkc import _lib as L
    q = dict(qbits=16, qh_exact=1, hq=True, U_h=True)
    assert _form(_args(L.CELL_LSTM, 512, 12, False, **q)) == (2, 2)
    # forward loops for H = 768 / 1024; their BPTT keeps the per-step launches (H = 512 only)
    assert _form(_args(L.CELL_LSTM, 1024, 16, False, **q)) == (2, 0)


def test_c3_ligru_fp32_grid_loops():
    from pkc import _lib as L
    assert _form(_args(L.CELL_LIGRU, 550, 8, True)) == (2, 2)     # C3: 16 rows
    assert _form(_args(L.CELL_LIGRU, 24, 4, False)) == (2, 2)
    assert _form(_args(L.CELL_LIGRU, 550, 9, True)) == (0, 0)     # 18 rows > 16
    assert _form(_args(L.CELL_LIGRU, 1024, 8, True)) == (0, 0)    # H > 768


@pytest.mark.parametrize("case", ["small_h", "too_many_rows", "layernorm", "block_sparse",
                                  "quant_not_exact", "gru"])
def test_per_step_fallbacks(case):
    from pkc import _lib as L
    a = {"small_h": lambda: _args(L.CELL_LSTM, 256, 16, True),
         "too_many_rows": lambda: _args(L.CELL_LSTM, 1024, 17, True),     # 34 rows > 32
         "layernorm": lambda: _args(L.CELL_LSTM, 1024, 16, True, ln_gamma=True),
         "block_sparse": lambda: _args(L.CELL_LSTM, 1024, 16, True, kmap_fwd=True, kmap_bwd=True),
         "quant_not_exact": lambda: _args(L.CELL_LSTM, 512, 12, False, qbits=16, hq=True),
         "gru": lambda: _args(L.CELL_GRU, 550, 8, True)}[case]()
    assert _form(a) == (0, 0)


def test_environment_switches(monkeypatch):
    from pkc import _lib as L
    # removed switches of retired kernel forms: setting them changes nothing
    for name, value in (("PKC_RNN_LSTM_F32_TL", "2"), ("PKC_RNN_LSTM_F32_LDS", "0"),
                        ("PKC_RNN_LSTM_F32_RS", "4")):
        monkeypatch.setenv(name, value)
        assert _form(_args(L.CELL_LSTM, 1024, 16, True)) == (2, 2)
        assert _form(_args(L.CELL_LSTM, 512, 12, False)) == (2, 2)
        assert _form(_args(L.CELL_LSTM, 768, 10, True)) == (2, 2)
        assert _form(_args(L.CELL_LSTM, 1024, 17, True)) == (0, 0)
    monkeypatch.setenv("PKC_RNN_LSTM_RS", "4")           # no longer a value of this switch
    assert _form(_args(L.CELL_LSTM, 1024, 16, True, step_bf16=1, hs_h=True, U_h=True,
                       ut_h=True, dgates_h=True)) == (2, 2)
    monkeypatch.setenv("PKC_RNN_LSTM_F32", "0")          # the fp32 LSTM loops only
    assert _form(_args(L.CELL_LSTM, 1024, 16, True)) == (0, 0)
    assert _form(_args(L.CELL_LSTM, 1024, 16, True, step_bf16=1, hs_h=True, U_h=True,
                       ut_h=True, dgates_h=True)) == (2, 2)
    monkeypatch.setenv("PKC_RNN_LSTM_PERSIST", "0")      # every LSTM loop
    assert _form(_args(L.CELL_LSTM, 1024, 16, True, step_bf16=1, hs_h=True, U_h=True,
                       ut_h=True, dgates_h=True)) == (0, 0)
    monkeypatch.setenv("PKC_RNN_LIGRU_GRID", "0")
    assert _form(_args(L.CELL_LIGRU, 550, 8, True)) == (0, 0)


# ------------------------------------------------------------------ form 1: the persistent liGRU loops
def _persist_args(H=550, B=8, bidir=True, **kw):
    """liGRU with bf16 step products, both plans and persist_kb = the forward slot count
    (pkc_rnn_persist_geometry): everything rnn_persist_ok asks for."""
    from pkc import _lib as L
    from pkc.engine import persist_geometry
    base = dict(step_bf16=1, hs_h=True, U_h=True, ut_h=True, dgates_h=True, persist_fwd=True,
                persist_bwd=True, persist_kb=persist_geometry()[1])
    base.update(kw)
    return _args(L.CELL_LIGRU, H, B, bidir, **base)


def test_form1_accepts_the_persistent_ligru_layers():
    from pkc.engine import persist_geometry
    hmax = persist_geometry()[4]
    assert _form(_persist_args()) == (1, 1)                          # C3
    assert _form(_persist_args(hmax, 3, False)) == (1, 1)            # the largest H, one direction
    assert _form(_persist_args(2, 1, False)) == (1, 1)
    assert _form(_persist_args(96, 17, True)) == (1, 1)              # 34 rows: no row limit
    assert _form(_persist_args(kmap_fwd=True, kmap_bwd=True)) == (1, 1)      # (tables beside plans)
    assert _form(_persist_args(dy_nslab=2, dy_slab_stride=1 << 20)) == (1, 1)


@pytest.mark.parametrize("case", ["H578", "odd_H", "persist_kb", "layernorm", "no_hs_h", "no_ut_h",
                                  "no_dgates_h", "no_plan_bwd", "fp32_steps", "lstm"])
def test_form1_refusals(case, monkeypatch):
    from pkc import _lib as L
    from pkc.engine import persist_geometry
    monkeypatch.setenv("PKC_RNN_LIGRU_GRID", "0")       # (what form 1 falls back to: per step)
    nsf = persist_geometry()[1]
    a, want = {
        "H578": lambda: (_persist_args(578), (0, 0)),
        "odd_H": lambda: (_persist_args(549), (0, 0)),
        "persist_kb": lambda: (_persist_args(persist_kb=nsf - 1), (0, 0)),
        "layernorm": lambda: (_persist_args(ln_gamma=True), (0, 0)),
        "no_hs_h": lambda: (_persist_args(hs_h=False), (0, 0)),
        # the BPTT's own operands: the forward loop does not need them
        "no_ut_h": lambda: (_persist_args(ut_h=False), (1, 0)),
        "no_dgates_h": lambda: (_persist_args(dgates_h=False), (1, 0)),
        "no_plan_bwd": lambda: (_persist_args(persist_bwd=False), (1, 0)),
        "fp32_steps": lambda: (_persist_args(step_bf16=0), (0, 0)),
        "lstm": lambda: (_args(L.CELL_LSTM, 550, 8, True, step_bf16=1, hs_h=True, U_h=True,
                               ut_h=True, dgates_h=True, persist_fwd=True, persist_bwd=True,
                               persist_kb=nsf), (0, 0)),
    }[case]()
    assert _form(a) == want


def test_form1_with_three_dy_slabs_keeps_the_forward_loop():
    """dy_nslab = 3: the BPTT loop sums two slabs at the most, so the forward stays form 1 and the
    BPTT takes the per-step launches (bf16 steps: no grid-synchronised liGRU form either)."""
    assert _form(_persist_args(dy_nslab=3, dy_slab_stride=1 << 20)) == (1, 0)
    assert _form(_persist_args(dy_nslab=2, dy_slab_stride=1 << 30)) == (1, 0)    # 32-bit offsets
