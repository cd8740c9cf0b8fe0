"""The reference's DEBUG range lines from the Python driver (flux_calculator.F90:879-881, 921-924,
949-951, 1011-1013): run(..., log=...) at verbosity_level DEBUG on the Baltic set-up writes one
line per received and sent field per phase with numpy's min / max of the coupler's arrays; at
STANDARD it writes none."""
import numpy as np
import pytest

import namelists
from namelists import regrid_matrices

pytestmark = pytest.mark.gpu

from fcx import driver  # noqa: E402
from fcx.setup import setup_from_namelist  # noqa: E402
from fcx.synthetic import SyntheticCoupler, corrections  # noqa: E402

GRIDS = (3001, 2999, 3011)


class RecordingCoupler(SyntheticCoupler):
    """keeps what get() filled as well as what put() took"""

    def get(self, name, time, out, which_grid=None):
        super().get(name, time, out, which_grid)
        self.got = getattr(self, "got", {})
        self.got[(name, time)] = np.array(out, copy=True)


def _run(level, log):
    text = namelists.MOM5_BALTIC.replace("num_timesteps = 3", "num_timesteps = 2\n  verbosity_level = %d" % level)
    setup = setup_from_namelist(text, mype=0, grid_size=GRIDS)
    assert setup.nml["verbosity_level"] == level
    eng = setup.engine(corrections=(20000101, corrections(GRIDS[0])), regrid=regrid_matrices(GRIDS))
    coupler = RecordingCoupler.for_setup(setup)
    try:
        driver.run(setup, eng, coupler, log=log)
    finally:
        eng.close()
    return setup, coupler


def test_debug_lines_hold_numpys_ranges_of_the_couplers_arrays():
    lines = []
    setup, coupler = _run(2, lines.append)
    steps = setup.nml["num_timesteps"]
    assert len(lines) == steps * (len(setup.input_field) + len(setup.output_field))
    seen = {}
    for ln in lines:
        what, name, rest = ln.split()[0], ln.split()[1], ln.split("range = ")[1].split()
        t = int(ln.split("runtime=")[1].split()[0])
        seen[(what, name, t)] = (float(rest[0]), float(rest[1]))
    assert len(seen) == len(lines)
    for (name, t), a in coupler.got.items():
        assert seen[("received", name, t)] == (float(np.min(a)), float(np.max(a))), (name, t)
    for (name, t), a in coupler.sent.items():
        assert seen[("sent", name, t)] == (float(np.min(a)), float(np.max(a))), (name, t)
    assert len(coupler.got) + len(coupler.sent) == len(lines)


def test_standard_verbosity_writes_nothing():
    lines = []
    _run(1, lines.append)
    assert lines == []
