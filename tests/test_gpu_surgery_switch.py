"""The engine's one gradient-surgery mode switch (mtsac_set_pcgrad / _cagrad / _gradnorm share it): the three
modes exclude one another, none of them replays a captured graph, and a rejected call changes nothing.  No
update step is run."""

from __future__ import annotations

import itertools

import pytest

from test_gpu_pcgrad import _engine

pytestmark = pytest.mark.gpu

MODES = ("pcgrad", "cagrad", "gradnorm")
# a call of the mode's setter that its own argument validation rejects (PCGrad has no such argument)
BAD = {"cagrad": dict(num_iterations=0), "gradnorm": dict(asymmetry=float("nan"))}


def _set(e, mode, on, **kw):
    getattr(e, f"set_{mode}")(on, **kw)


@pytest.mark.parametrize("a,b", list(itertools.permutations(MODES, 2)))
def test_modes_exclude_one_another(a, b):
    from mtrl_amd._lib import MTSACError

    e = _engine(3, 32, 4)
    _set(e, a, True)
    with pytest.raises(MTSACError, match="-16"):
        _set(e, b, True)
    with pytest.raises(MTSACError, match="-95"):
        e.enable_graph(True)
    _set(e, a, False)
    _set(e, b, True)
    _set(e, b, False)
    e.close()


@pytest.mark.parametrize("a", list(BAD))
def test_rejected_call_changes_nothing(a):
    from mtrl_amd._lib import MTSACError

    other = next(m for m in MODES if m != a)
    # from no mode: the graph flag stays usable, another mode can go on
    e = _engine(3, 32, 4)
    e.enable_graph(True)
    with pytest.raises(MTSACError, match="-22"):
        _set(e, a, True, **BAD[a])
    e.enable_graph(True)
    e.close()
    e = _engine(3, 32, 4)
    e.enable_graph(True)
    with pytest.raises(MTSACError, match="-22"):
        _set(e, a, True, **BAD[a])
    _set(e, other, True)
    _set(e, other, False)
    e.enable_graph(True)
    e.close()
    # with the mode on: it stays on, and leaving it still gives the graph flag back
    e = _engine(3, 32, 4)
    e.enable_graph(True)
    _set(e, a, True)
    with pytest.raises(MTSACError, match="-22"):
        _set(e, a, True, **BAD[a])
    with pytest.raises(MTSACError, match="-16"):
        _set(e, other, True)
    with pytest.raises(MTSACError, match="-95"):
        e.enable_graph(True)
    _set(e, a, False)
    e.enable_graph(True)
    e.close()
