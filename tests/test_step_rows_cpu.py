"""tests/step_rows.py names one handle configuration per compiled step kernel.  Here, without a
GPU: plan_step (csrc/mev_plan.h, through tests/native/step_plan_check.cpp's `rows`) sends every
entry's shape to the entry's row, and the entries cover every row of kStepKeys and kServeKeys,
each with and without the distance table, as `keys` prints the tables -- so a change of the plan
or of the tables that strands a kernel without a test fails here."""
import subprocess

import edge_poses as EP
import native_build
import step_rows as SR


def _run(*args, stdin=None):
    exe = native_build.build("step_plan_check")
    r = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def _tables():
    keys = {"step": [], "serve": []}
    for ln in _run("keys"):
        f = ln.split()
        assert int(f[1]) == len(keys[f[0]])
        keys[f[0]].append(tuple(int(x) for x in f[2:]))
    return keys


def test_every_entry_lands_on_its_row():
    out = _run("rows", stdin="".join(SR.shape_line(e) + "\n" for e in SR.ENTRIES))
    assert len(out) == len(SR.ENTRIES)
    keys = _tables()
    for e, ln in zip(SR.ENTRIES, out):
        wc, step, serve = (int(x) for x in ln.split("|")[-1].split())
        path = int(ln.split("|")[1].split()[0])
        if e["table"] == "step":
            assert path == 2 and step == e["row"], (e["name"], ln)
            assert wc == keys["step"][step][-1], (e["name"], ln)
        else:
            assert serve == e["row"], (e["name"], ln)
        assert e["E"] <= 64
        if e["traffic"] and e["table"] == "step" and e["row"] in (0, 1):
            assert e["E"] % 16 == 0


def test_entries_cover_every_row_of_both_tables():
    keys = _tables()
    assert len(keys["step"]) >= 35 and len(keys["serve"]) >= 6
    want = {(t, r, tab) for t in keys for r in range(len(keys[t])) for tab in (0, 1)}
    have = {(e["table"], e["row"], e["tab"]) for e in SR.ENTRIES}
    assert not (have & set(SR.UNREACHABLE)), "an entry reaches a row listed as unreachable"
    missing = sorted(want - have - set(SR.UNREACHABLE))
    assert not missing, f"kernel rows without an entry in tests/step_rows.py: {missing}"
    assert not (have | set(SR.UNREACHABLE)) - want, "entries for rows the tables do not hold"
    # only the TAB slots of WC rows may be unreachable (they hold the plain kernel)
    for t, r, tab in SR.UNREACHABLE:
        assert t == "step" and tab == 1 and keys["step"][r][-1] == 1, (t, r, tab)
    assert len({e["name"] for e in SR.ENTRIES}) == len(SR.ENTRIES)
    # every fixture recorded from the reference (tests/golden/edge_*.npz) is some fused entry's configuration,
    # so tests/test_edge_rows_gpu.py steps its pose sets through a k_step row, not only through k_cars + k_lidar
    fused = {EP.fixture_for(e) for e in SR.ENTRIES if e["table"] == "step"}
    assert set(EP.fixture_names()) <= fused, set(EP.fixture_names()) - fused
    print(f"{len(SR.ENTRIES)} entries, {len(SR.UNREACHABLE)} unreachable slots, "
          f"{len(keys['step'])} k_step rows, {len(keys['serve'])} k_serve rows")
