#!/usr/bin/env python3
"""Writes RESULTS.md: every key of the driver's bench line -> the number of the round's evidence run, the command that prints
it and the ONE file under profiles/ that holds it.  Reads only committed files (profiles/r06_*.json); run from anywhere:
    python tools/make_results.py          (after tools/exp/r06_final.sh's outputs were copied to profiles/)"""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = os.path.join(ROOT, "profiles")
TAG = "r06"


def line(name):
    try:
        return json.loads(open(os.path.join(P, name)).read().strip().splitlines()[-1])
    except Exception:   # noqa: BLE001
        return None


def k(x):
    return f"{x / 1e3:.1f} k"


def main():
    b = line(f"{TAG}_bench.json")
    nb = line(f"{TAG}_bench_no_preheat.json")
    sq = line(f"{TAG}_bench_sequential.json")
    k4 = line(f"{TAG}_bench_4k.json")
    rr = line(f"{TAG}_bench_4k_roundrobin.json")
    rh = line(f"{TAG}_bench_rehearsal_3ranks_one_gpu.json")
    la = line(f"{TAG}_bench_launcher_1rank_rccl.json")
    r, ss, cw = b["roofline"], b["steady_state"], b["cold_start_window"]
    rows = []

    def row(key, val, cmd, f):
        rows.append(f"| `{key}` | {val} | `{cmd}` | `profiles/{f}` |")

    D = "python bench.py --full --steps 20 --warmup 5"
    F = f"{TAG}_bench.json"
    row("value, ms_per_step", f"**{k(b['value'])} frames/s, {b['ms_per_step']} ms per 256-frame step** (behind {b['preheat']['seconds']} s = "
        f"{b['preheat']['steps']} untimed steps of the same load)", "python bench.py --steps 20 --warmup 5  (the driver's command; --full: the rest)", F)
    row("roofline.frac", f"**{r['frac']}** of 8 TB/s on the ALGORITHMIC 2N + 5P = {r['algorithmic_bytes_per_launch'] / 1e9:.4f} GB per launch "
        f"(not HBM utilisation: `frac_note`)", D, F)
    row("roofline.traffic, frac_actual, frac_of_achievable", f"{(r['traffic'] or 0) / 1e9:.4f} GB per launch by the counters "
        f"({r.get('traffic_over_algorithmic')} of the algorithmic bytes) -> **{r.get('frac_actual')} of 8 TB/s nominal, "
        f"{r.get('frac_of_achievable')} of this board's streaming read** ({b['board']['hbm_stream_read_gbps']:.0f} GB/s)", D, F + "`, counters: `profiles/pmc_summary.json")
    row("cold_start_window", f"{k(cw['value'])} frames/s, {cw['ms_per_step']} ms, frac {cw['frac']}: the same 5 + 20 steps as the first GPU work of "
        f"the process (rounds 1-5's `value`)", D, F)
    if nb:
        row("value with --preheat-s 0", f"{k(nb['value'])} frames/s, {nb['ms_per_step']} ms, frac {nb['roofline']['frac']} (later in the same call: a warm chip)",
            D + " --preheat-s 0 ...", f"{TAG}_bench_no_preheat.json")
    di = line(f"{TAG}_bench_default_invocation.json")
    if di:
        row("the default invocation (100 timed steps, 10 warm-up; later in the call: a warm chip)", f"{k(di['value'])} frames/s, {di['ms_per_step']} ms, frac "
            f"{di['roofline']['frac']} / actual {di['roofline'].get('frac_actual')} / of achievable {di['roofline'].get('frac_of_achievable')}; steady_state {di['steady_state']['frac']}",
            "python bench.py --full", f"{TAG}_bench_default_invocation.json")
    try:
        runs = [ln for ln in open(os.path.join(P, "r06q_eighteen_seconds.txt")).read().splitlines() if ln.startswith("run ")]
        vals = [(float(ln.split()[2]), float(ln.split()[4]), float(ln.split()[7])) for ln in runs]
        row("sustained over 18 s (40 000 timed steps, twice in a row on one box)", " then ".join(f"{k(v[0])} frames/s, {v[1]} ms, frac {v[2]}" for v in vals),
            "python bench.py --steps 40000 --warmup 10 --preheat-s 0 ...", "r06q_eighteen_seconds.txt")
    except Exception:   # noqa: BLE001
        pass
    row("steady_state", f"{k(ss['frames_per_s'])} frames/s, {ss['ms_per_step']} ms, frac {ss['frac']} / actual {ss.get('frac_actual')} / of achievable "
        f"{ss.get('frac_of_achievable')} (1000 more steps behind the timed ones)", D, F)
    row("roofline.kernels[].avg_us", " / ".join(f"{x['avg_us']}" for x in r["kernels"]) + " µs: pack (two launches, the later end) / index / expansion, "
        "beside each other (pipelined)", D, F + f"`, trace: `profiles/{TAG}_kernel_stats.csv")
    if sq:
        row("the same, one batch after the other", f"{k(sq['value'])} frames/s, {sq['ms_per_step']} ms, frac {sq['roofline']['frac']}; kernels "
            + " / ".join(f"{x['avg_us']}" for x in sq["roofline"]["kernels"]) + " µs", "MI355_PIPELINE=0 " + D + " ...", f"{TAG}_bench_sequential.json")
    row("two_streams_one_gpu", f"{k(b['two_streams_one_gpu']['frames_per_s'])} frames/s aggregate, frac {b['two_streams_one_gpu']['frac']}", D, F)
    pm = b["pair_mode"]
    row("pair_mode", f"frac {pm['frac']} (own stream) / {pm['frac_sequential']} (caller's stream); kernels {pm['kernels_us']} µs; P = {pm['changed_bytes_per_frame']:.0f} per frame", D, F)
    rg = b["regimes"]
    s0 = rg["S0_refrand_pairs"]
    row("regimes.S0_refrand_pairs", f"**frac {s0['frac']}**, kernels {s0['kernels_us']} µs, output arrays from `mi355_alloc_outputs` "
        f"({rg['outputs']['value_arrays_drawn']} value array(s) drawn, {rg['outputs']['ms']} ms); `plain_allocation` (two torch.empty arrays, this "
        f"process's lot): frac {s0['plain_allocation']['frac']}, kernels {s0['plain_allocation']['kernels_us']}", D, F + f"`; 8 fresh processes: `profiles/r06f_alloc_outputs_eight_processes.txt")
    row("regimes.P_eq_N_pairs / P_eq_0_pairs", f"frac {rg['P_eq_N_pairs']['frac']} ({rg['P_eq_N_pairs']['kernels_us']} µs) / {rg['P_eq_0_pairs']['frac']}", D, F)
    c3, c4, md = b["config3"], b["config4"], b["median5x5"]
    row("config3 (BASELINE configs[2])", f"{c3['us_per_frame']} µs per frame own stream / {c3['sequential_us_per_frame']} caller's stream, frac {c3['frac']} on 3N + 5P "
        f"(the one-read form measured and removed: 4.96 against 4.91 µs)", D, F + "`; one-read A/B: `profiles/r06d_config3_one_read.txt")
    row("config4 (BASELINE configs[3])", f"{c4['us_per_frame']} / {c4['sequential_us_per_frame']} µs per frame, frac {c4['frac']} on 5N + 5P", D, F + f"`; per kernel: `profiles/{TAG}_filters_kernel_stats.csv")
    row("median5x5", f"{md['us_per_frame']} µs per frame (VALU-bound)", D, F)
    c5 = b["config5_per_gpu"]
    row("config5_per_gpu (BASELINE configs[4], one GPU's share)", f"{k(c5['frames_per_s'])} 4K frames/s, frac {c5['frac']} / {c5['frac_sequential']}", D, F)
    if rr:
        row("the same shape as the whole job", f"{k(rr['value'])} 4K frames/s, {rr['ms_per_step']} ms per 64 pairs, frac {rr['roofline']['frac']}",
            D + " --width 3840 --height 2160 --batch 64 --shard roundrobin ...", f"{TAG}_bench_4k_roundrobin.json")
    if k4:
        row("4K stream", f"{k(k4['value'])} frames/s, frac {k4['roofline']['frac']}", D + " --width 3840 --height 2160 --batch 64 ...", f"{TAG}_bench_4k.json")
    hp = b["host_path"]
    row("host_path", f"{hp['frames_per_s']} frames/s blocking, {hp['pipelined_frames_per_s']} pipelined ({hp['pcie_h2d_gbps']} GB/s of PCIe uploads); never `value`", D, F)
    cb = b["cpu_baseline"]
    ref = cb.get("reference_filter_chain") or {}
    row("cpu_baseline", f"{cb['value']} frames/s on 1 core (oracle, `kind: port`); {cb['all_cores']['value']} on {cb['all_cores']['cores']} threads; the reference's own "
        f"`server.cpp` CPU branch {ref.get('value')}", D, F)
    row("parity", ("all true: " if all(b["parity"].values()) else "FAILED: ") + ", ".join(b["parity"]), D, F)
    bd = b["board"]
    row("board", f"shader {bd['shader_mhz_under_valu_load']:.0f} MHz under load; streaming read {bd['hbm_stream_read_gbps']:.0f}, write {bd['hbm_stream_write_gbps']:.0f}, "
        f"index + value per lane {bd['hbm_narrow_write_gbps']:.0f} GB/s", D, F)
    if la:
        c = la["config5"]
        L = "python -m torch.distributed.run --nproc-per-node=1 ... bench.py --gpus 1 --full --steps 20 --warmup 5 ..."
        G = f"{TAG}_bench_launcher_1rank_rccl.json"
        row("N = 1 under the launcher, real RCCL: value", f"{k(la['value'])} frames/s, {la['ms_per_step']} ms (`config.core_flags`: MI355_FLAG_OWN_QUEUES; without the "
            "flag: 462 k)", L, G + "`; the finding: `profiles/r06k_streams_and_hardware_queues.txt")
        row("... ranks_seen, gather_ms, gather_bytes, gather_verified, final_gather_ms, value_with_final_gather",
            f"{la['ranks_seen']}, {la['gather_ms']} ms, {la['gather_bytes']} B, {la['gather_verified']}, {la.get('final_gather_ms')} ms, {k(la.get('value_with_final_gather') or 0)}", L, G)
        row("... config5 (BASELINE configs[4] across the ranks)", f"{k(c['value'])} 4K frames/s, {c['ms_per_step']} ms per pass, frac {c['frac']}, per rank {c['frac_per_rank']}; "
            f"gather {c['final_gather_ms']} ms, {c['gather_bytes']} B, {c['gather_gbps']} GB/s (device-to-device at N = 1); parity {c['parity']}, gather_verified {c['gather_verified']}", L, G)
    if rh:
        c = rh["config5"]
        row("N = 3 rehearsal on ONE GPU (NOT a measurement)", f"ranks_seen {rh['ranks_seen']}, gather_verified {rh['gather_verified']}, config5: parity {c['parity']}, "
            f"gather_verified {c['gather_verified']}, ranks_seen {c['ranks_seen']}, {c['gather_bytes']} B gathered",
            "python bench.py --gpus 3 --rehearse-on-one-gpu --full --batch 64 ...", f"{TAG}_bench_rehearsal_3ranks_one_gpu.json")
    head = f"""# RESULTS — every key of the bench line, the command that prints it, the one file that holds it

Generated by `tools/make_results.py` from the committed outputs of two `gpurun` calls, a 1×MI355X box each: `tools/exp/r06_final.sh`
(GPU suite, `smoke()`, `tests/soak.py 3000`, `tests/soak_chain.py 60`, every line below but the first command's, the `rocprofv3`
passes) and, once that call's counters were committed as `profiles/pmc_summary.json`, `tools/exp/r06_final2.sh` (the whole GPU
suite again: 270 passed; the first command, `profiles/{TAG}_bench.json`; `python bench.py` without arguments,
`profiles/{TAG}_bench_default_invocation.json`: 100 timed steps on a chip that had been working for minutes -- the warm,
sustained figure).  Log of both: `profiles/{TAG}_final_log.txt`.  Boxes differ by ±5 % and a chip's state by more (DESIGN.md §6, §8): `BENCH_r06.json`, the driver's own run of
the first command on another box, will differ in the digits, not in the keys.  Experiments of the round (what was tried, kept,
removed): `profiles/README.md` "Round 6"; rounds 1-5: `profiles/README.md` / `profiles/archive/`.

| key of the line | this run | command | file |
|---|---|---|---|
"""
    tail = f"""
Reading the three fractions of the headline: `frac` {r['frac']} is the contract's figure (algorithmic bytes / time / 8 TB/s) and can
pass 1 because the stream kernel reads N where the model counts 2N; the chip itself moved {r.get('traffic_over_algorithmic')} of those bytes, i.e.
`frac_actual` {r.get('frac_actual')} of the nominal 8 TB/s, which is `frac_of_achievable` {r.get('frac_of_achievable')} of what a plain streaming read reaches on
this board.  The first GPU work of a process (`cold_start_window`, {cw['frac']}) sits on the chip's clock ramp; `value` and `steady_state`
do not.

N > 1: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N
--steps K --warmup W` (the driver's command) prints the same keys with `n_gpus` N, `value` = all ranks' frames / MAX over the
ranks of the K steps, `value_with_final_gather`, `gather_*`, and with `--full` `gather_every` and the `config5` object (4K sequence dealt
round-robin over the N ranks + RCCL gather to rank 0, parity on rank 0's copy).  No 8-GPU node was available to the builder:
the N = 3 line above is a rehearsal on one GPU, the N = 1 line runs the same code over real RCCL.
"""
    open(os.path.join(ROOT, "RESULTS.md"), "w").write(head + "\n".join(rows) + "\n" + tail)
    print(f"RESULTS.md: {len(rows)} rows")


if __name__ == "__main__":
    main()
