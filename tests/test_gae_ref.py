"""mev_gae's arithmetic on the host: csrc/mev_gae.h's gae_step -- the text k_gae compiles -- run by
tests/native/gae_check.cpp over a hand-computed 3-step example (asserted there) and fixed pseudo-random
tables, against actor_critic_ref.gae_ref on the printed inputs, bit for bit.  gae_ref itself is checked
against a float64 restatement within 1e-5 relative: a sanity check, not the contract."""
import subprocess

import numpy as np

import actor_critic_ref as AC
import native_build


def _cases(text):
    cases, cur = [], None
    for line in text.splitlines():
        tag, *rest = line.split()
        if tag == "CASE":
            cur = dict(name=rest[0], T=int(rest[1]), E=int(rest[2]), N=int(rest[3]),
                       gamma=np.array([int(rest[4], 16)], np.uint32).view(np.float32)[0],
                       lam=np.array([int(rest[5], 16)], np.uint32).view(np.float32)[0], mask=bool(int(rest[6])))
            cases.append(cur)
        elif tag in ("R", "V", "ADV", "RET"):
            cur[tag] = np.array([int(x, 16) for x in rest], np.uint32).view(np.float32)
        elif tag in ("D", "TE", "TR", "EB", "VALID"):
            cur[tag] = None if rest == ["-"] else np.array([int(x) for x in rest], np.uint8)
    return cases


def _run():
    exe = native_build.build("gae_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert "GAE CHECK OK" in r.stdout
    return _cases(r.stdout)


def _shaped(c):
    T, E, N = c["T"], c["E"], c["N"]
    sh = lambda a, s: None if a is None else a.reshape(s)
    return dict(reward=c["R"].reshape(T, E, N), value=c["V"].reshape(T + 1, E, N), done=sh(c["D"], (T, E, N)),
                terminated=sh(c["TE"], (T, E)), truncated=sh(c["TR"], (T, E)), ended_before=c["EB"], gamma=c["gamma"],
                lam=c["lam"], mask_reset_steps=c["mask"])


def test_gae_step_matches_gae_ref_bit_for_bit():
    cases = _run()
    assert len(cases) == 24
    seen = set()
    for n, c in enumerate(cases):
        kw = _shaped(c)
        adv, ret, valid = AC.gae_ref(**kw)
        tag = f"case {n}: T={c['T']} E={c['E']} N={c['N']} gamma={c['gamma']} lam={c['lam']} mask={c['mask']}"
        assert np.array_equal(adv.reshape(-1).view(np.uint32), c["ADV"].view(np.uint32)), tag + ": advantages"
        assert np.array_equal(ret.reshape(-1).view(np.uint32), c["RET"].view(np.uint32)), tag + ": returns"
        assert np.array_equal(valid.reshape(-1), c["VALID"]), tag + ": valid"
        seen.add((c["D"] is not None, c["TE"] is not None, c["TR"] is not None, c["EB"] is not None, c["mask"]))
        if c["mask"] and c["T"] > 1:
            assert (valid == 0).any() and (valid == 1).any(), tag
    assert len(seen) == 4  # every option set of the tables ran


def test_gae_ref_against_float64():
    for c in _run():
        kw = _shaped(c)
        adv, ret, _ = AC.gae_ref(**kw)
        adv64, ret64 = AC.gae_ref64(**kw)
        # relative to the magnitudes that enter a row: |r| <= 2, |V| <= 30, and a trace of up to T such rows
        scale = 62.0 * c["T"]
        assert np.max(np.abs(adv - adv64)) <= 1e-5 * scale
        assert np.max(np.abs(ret - ret64)) <= 1e-5 * scale
