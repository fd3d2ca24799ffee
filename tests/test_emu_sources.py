"""tests/emu_backend.py rebuilds libppg_emu.so when a file it watches is newer than the library.  Every file the two emulator units
reach through quoted includes must be watched, or an edit to a kernel header is tested against the old binary.  The walk below is
this test's own (a stack and a regular expression), not the one emu_backend uses."""
import os
import re

from tests import emu_backend


def _reached(units):
    todo, seen = [os.path.join(emu_backend.EMU_DIR, u) for u in units], set()
    while todo:
        path = os.path.normpath(todo.pop())
        if path in seen:
            continue
        seen.add(path)
        with open(path) as f:
            todo += [os.path.join(os.path.dirname(path), inc) for inc in re.findall(r'#\s*include\s*"([^"]+)"', f.read())]
    return seen


def test_every_file_the_emulator_units_include_is_checked_for_staleness():
    reached = _reached(("ppg_emu.cpp", "ppg_emu_part.cpp"))
    assert any(p.endswith("ppg_backward.h") for p in reached) and any(p.endswith("wave_emu.h") for p in reached)
    watched = {os.path.normpath(p) for p in emu_backend.sources()}
    assert not sorted(os.path.relpath(p, emu_backend.ROOT) for p in reached - watched)
