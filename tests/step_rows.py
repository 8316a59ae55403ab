"""One handle configuration per compiled step kernel: every row of kStepKeys and kServeKeys
(csrc/mev_plan.h), each with the probe distances computed (TAB off) and read from a table (TAB
on).  An entry is the smallest configuration that reaches its row at E <= 64: the explicit
set_step_kernel / set_step_pack / set_step_split calls (an explicit pack makes the early split
independent of E; the traffic split needs E % 16 == 0), obs_dim, MEV_NO_WORLD_CONST in the
environment at creation, lidar_step 4.0 (exact multiples, no table) or 3.3 (accumulated, a
table), max_npcs and per-car sizes (set_car_dims).

tests/test_step_rows_cpu.py feeds shape_line(entry) to `step_plan_check rows` and asserts that
the plan lands on the entry's row, and that the entries and UNREACHABLE together are every
(row, TAB) of both tables as `step_plan_check keys` prints them.  tests/test_edge_rows_gpu.py
creates each entry's handle, asserts Handle.step_row() and steps it from the edge poses."""
from __future__ import annotations

OBS_HEAD = 31
REF = dict(lanes=3, fov=360.0, max_dist=250.0, lidar_step=4.0)  # the reference's world (csrc/mev_refworld.h)
DEFAULTS = dict(E=64, n=8, rays=64, traffic=0, max_npcs=32, obs_dim=0, pack=0, split=0, kernel=2, dims=False,
                no_world_const=False, serve=False, note="", **REF)
TAB_STEP = 3.3  # multiples of 3.3 are not the accumulated sums (Lidar.cpp:33): the kernels read a table


def _e(table, row, name, **kw):
    """One entry per TAB: lidar_step 4.0 and 3.3.  (A handle with a table is not the reference's
    world, so its key never has wc: the two WC rows have no reachable TAB slot, UNREACHABLE.)"""
    out = []
    for tab in (0, 1):
        d = dict(DEFAULTS, table=table, row=row, tab=tab, name=f"{table}{row:02d}_{name}_{'tab' if tab else 'mul'}", **kw)
        if table == "serve":
            d["serve"], d["kernel"] = True, 0
        if tab:
            d["lidar_step"] = TAB_STEP
        out.append(d)
    return out


def _entries():
    T = dict(traffic=1, n=1)
    s = []
    # ---- k_step, in kStepKeys' order
    s += _e("step", 0, "traffic_split_r64", **T)
    s += _e("step", 1, "traffic_split_r32", rays=32, **T)
    s += _e("step", 2, "traffic_one_wave", split=1, **T)
    s += _e("step", 3, "traffic_n2_runtime", traffic=1, n=2)
    s += _e("step", 4, "traffic_k64_runtime", max_npcs=64, **T)
    s += _e("step", 5, "esplit_pack8", n=1, pack=8)
    s += _e("step", 6, "esplit_pack4_r64_n1", n=1, pack=4)
    s += _e("step", 7, "esplit_pack4_r32_n1", n=1, rays=32, pack=4)
    s += _e("step", 8, "esplit_pack4_n2", n=2, pack=4)
    s += _e("step", 9, "esplit_pack2_r96_n1", n=1, rays=96, pack=2)
    s += _e("step", 10, "esplit_pack2_r64_n1", n=1, pack=2)
    s += _e("step", 11, "esplit_pack2_n2", n=2, pack=2, lanes=2)
    s += _e("step", 12, "esplit_pack1", n=8, pack=1, split=3)
    s += _e("step", 13, "split_pack8", n=1, pack=8, split=2)
    s += _e("step", 14, "split_pack4", n=2, pack=4, split=2)
    s += _e("step", 15, "split_pack2", n=3, pack=2, split=2)
    s += _e("step", 16, "split_8x64_lanes2", split=2, lanes=2)
    s += _e("step", 17, "split_8x96", rays=96, split=2)
    s += _e("step", 18, "split_8x128", rays=128, split=2)
    s += _e("step", 19, "split_n1", n=1, pack=1, split=2, lanes=2)
    s += _e("step", 20, "split_n4", n=4, pack=1, split=2)
    s += _e("step", 21, "wave_pack8", n=1, pack=8, split=1)
    s += _e("step", 22, "wave_pack4", n=2, pack=4, split=1)
    s += _e("step", 23, "wave_pack2", n=4, pack=2, split=1, rays=48)
    # (the reference's world, but rows wider than 31 + R: launch_step drops wc)
    s += _e("step", 24, "wave_8x64_wide_rows", split=1, obs_dim=127)
    s += _e("step", 25, "wave_n4_r64", n=4, pack=1, split=1)
    s += _e("step", 26, "wave_8x96", rays=96, split=1)
    s += _e("step", 27, "wave_n5_r96", n=5, rays=96, pack=1, split=1)
    s += _e("step", 28, "wave_8x128_no_world_const", rays=128, split=1, no_world_const=True)
    s += _e("step", 29, "wave_n3_r128", n=3, rays=128, pack=1, split=1)
    # (128 beams of which the observation keeps 96: a multiple of 64 that is no compile-time count)
    s += _e("step", 30, "wave_8x128_obs127", rays=128, split=1, obs_dim=127)
    s += _e("step", 31, "wave_8x48_lanes2", rays=48, split=1, lanes=2)
    s += _e("step", 32, "runtime_n12_r96", n=12, rays=96, fov=120.0, max_dist=180.0)
    s += [dict(d, name=d["name"].replace("n12_r96", "8x128_dims"), n=8, rays=128, dims=True, fov=360.0, max_dist=250.0)
          for d in _e("step", 32, "runtime_n12_r96")]
    # (WC: the reference's world and plain rows at compile time; the TAB slot holds the plain kernel,
    # rows 24 / 28 with TAB, and no plan reaches it)
    s += _e("step", 33, "wave_8x64_world", split=1)[:1]
    s += _e("step", 34, "wave_8x128_world", rays=128, split=1)[:1]
    # ---- k_serve, in kServeKeys' order (host-mode steps of a handle whose outputs fit the pinned
    # block, 256 KB: fewer envs where 64 do not)
    s += _e("serve", 0, "traffic", **T)
    s += _e("serve", 1, "traffic_k64", max_npcs=64, **T)
    s += _e("serve", 2, "n1", n=1)
    s += _e("serve", 3, "8x64")
    s += _e("serve", 4, "8x96", rays=96, E=48)
    s += _e("serve", 5, "8x128_unspecialised", rays=128, E=48)[:1] + _e("serve", 5, "n4_r48", n=4, rays=48, lanes=2)[1:]
    return s


ENTRIES = _entries()
# (table, row, tab) that no plan produces, with the reason
UNREACHABLE = {
    ("step", 33, 1): "a WC row's TAB slot holds the plain kernel (row 24's): a handle with a distance table is not "
                     "the reference's world, so plan_step never sets wc for it",
    ("step", 34, 1): "a WC row's TAB slot holds the plain kernel (row 28's): a handle with a distance table is not "
                     "the reference's world, so plan_step never sets wc for it",
}


def obs_width(e) -> int:
    return e["obs_dim"] if e["obs_dim"] > 0 else OBS_HEAD + e["rays"]


def shape_line(e) -> str:
    """The entry as `step_plan_check rows` reads it: E N R K lidar_slots traffic dims step_kernel
    step_pack step_split world plain."""
    D = obs_width(e)
    world = int(not e["no_world_const"] and not e["dims"] and all(e[k] == v for k, v in REF.items()))
    plain = int(D == OBS_HEAD + e["rays"])
    return (f"{e['E']} {e['n']} {e['rays']} {e['max_npcs']} {min(e['rays'], D - OBS_HEAD)} {e['traffic']} "
            f"{int(e['dims'])} {e['kernel']} {e['pack']} {e['split']} {world} {plain}")


def config(e) -> dict:
    """mev_create's configuration of the entry (respawn off)."""
    c = dict(num_envs=e["E"], num_agents=e["n"], num_lanes=e["lanes"], lidar_rays=e["rays"], lidar_fov_deg=e["fov"],
             lidar_max_dist=e["max_dist"], lidar_step=e["lidar_step"], obs_dim=e["obs_dim"], respawn_enabled=0,
             max_npcs=e["max_npcs"])
    if e["traffic"]:
        c.update(traffic_flow=1, traffic_density=0.0)
    return c
