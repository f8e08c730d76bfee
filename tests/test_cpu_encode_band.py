"""Knob encode_band (HIC_KNOB_ENCODE_BAND, 16): the fused encoder's stacked bands
with the halo exchange are the default; 0 selects one unit per wave.  encode_order
keeps its values and its default.  No GPU call."""
import pytest

from hiccup_amd import _lib


def test_encode_band_default_and_range():
    assert _lib.get_knob("encode_band") == 1
    assert _lib.get_knob("encode_order") == 6
    with _lib.knobs(encode_band=0):
        assert _lib.get_knob("encode_band") == 0
        assert _lib.get_knob("encode_order") == 6
    assert _lib.get_knob("encode_band") == 1
    for bad in (2, 8, -2):
        with pytest.raises(ValueError):
            _lib.set_knob("encode_band", bad)
    assert _lib.load().hic_set_knob(16, -1) == _lib.HIC_OK
    assert _lib.load().hic_set_knob(17, 0) == _lib.HIC_ERR_ARG
