"""The script of tests/test_throttle_events_gpu.py::test_throttle_events_between_sweeps on the oracle alone, without an engine: the
choice of `big`, `other` and `small`, the fourteen sweeps, and that EVERY event is non-vacuous — `used.count` of a responsible row
or a summary word differs from the sweep before, a threshold edit flips a throttled flag and the last entry of the three-entry batch
flips it back, the copies' `used` is their originals', the deleted rows' columns are zero.  (The scan forms differ only on the
engine: to the oracle they are 8 and 16 dimensions.)"""
import pytest

from test_throttle_events_gpu import throttle_events


@pytest.mark.parametrize("form", ["one-chunk", "sixteen-dims"])
def test_every_throttle_event_moves_the_oracle(form, oracle_mod, monkeypatch):
    seen = throttle_events(form, oracle_mod, monkeypatch, gpu=False)
    assert len(seen) == 14
