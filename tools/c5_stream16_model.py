#!/usr/bin/env python3
"""CPU cost model for the C5 design DESIGN 8.3 left open: a 16-wave
`k_stream` with 4 KiB rounds whose payload phase batches two rounds' payloads per step.
Build it only if this predicts <= 38 us from a graph (frac >= 0.51) for C5 (1 M packed
Zipf(1.1) payloads, 142.1 MB + 12 B metadata each = 154.7 MB read).

Per-round operation counts come from the shipped source (csrc/crc32_stream.hpp k_stream,
stag_apply3x = 4 v_perm + 4 ds_read_b32 + 2 v_xor3; nib_apply = 8 v_bfe + 8 address
adds + 8 ds_read_b32 + 4 xor; one dependent LDS round trip per apply).  Three limits per
design, each calibrated on a kernel measured on the same part:

  VALU   wave-instructions per CU / (1 per cycle per CU: four SIMDs, 4 cycles per wave64
         op) / u_v, u_v = 0.80 (k_pieces' SQ_ACTIVE_INST_VALU share on C5, the best any
         mixed-length kernel reached, profiles/r05/c5_counters_tailclamp_ab.json)
  LDS    issue cycles per CU (ds_read/write_b32 2 cycles per wave op at 128 B/clk, b128
         8) / u_l, u_l = 0.48 (k_pieces' measured LDS busy share)
  chain  per wave: rounds x dependent LDS round trips x L.  L is calibrated so that the
         shipped 8-wave k_stream's chain limit equals its measured 57.1 us (graph);
         at 16 waves L is scaled by the LDS queue's load (its issue cycles per unit
         time), never below the unloaded ~130 cycles
The prediction is prologue (5.5 us, measured entry -> first round) + max of the three.
Writes JSON to stdout (profiles/r06/c5_stream16_model.json).
"""
import json

CLK = 2.4e9
CUS = 256
PAYLOAD = 142_102_337          # C5 Zipf(1.1), 1 M packets (configs leg, BENCH)
READ = PAYLOAD + 12 * (1 << 20)
NPAY = 1 << 20
PROLOGUE_US = 5.5              # entry -> first round (pprobe)
U_V, U_L = 0.80, 0.48
MEASURED = {"k_pieces": 42.9, "k_stream8": 57.1}   # us from a graph (profiles/r05final, r06a)

APPLY = {"valu": 6, "lds_b32": 4, "depth": 1}       # stag_apply3(x)
NIB = {"valu": 20, "lds_b32": 8, "depth": 1}        # nib_apply + the shuffle / select around it


def phase(n_apply=0, n_nib=0, valu=0, b32=0, b128=0, depth=0):
    return {"valu": n_apply * APPLY["valu"] + n_nib * NIB["valu"] + valu,
            "lds_b32": n_apply * APPLY["lds_b32"] + n_nib * NIB["lds_b32"] + b32,
            "lds_b128": b128, "depth": n_apply * APPLY["depth"] + n_nib * NIB["depth"] + depth}


def total(phases, mult=None):
    mult = mult or {}
    out = {"valu": 0.0, "lds_b32": 0.0, "lds_b128": 0.0, "depth": 0.0}
    for k, p in phases.items():
        m = mult.get(k, 1.0)
        for f in out:
            out[f] += m * p[f]
    return out


def design(name, round_bytes, waves, phases, steps_per_round):
    """steps_per_round: payload steps (<= 64 payloads each) per round."""
    per = total(phases, {"payload": steps_per_round})
    rounds = READ / round_bytes                # over the chip (metadata bytes folded in, as measured frac does)
    lds_cyc = per["lds_b32"] * 2 + per["lds_b128"] * 8
    valu_us = rounds * per["valu"] / CUS / CLK * 1e6 / U_V
    lds_us = rounds * lds_cyc / CUS / CLK * 1e6 / U_L
    rounds_per_wave = rounds / (CUS * waves)
    return {"design": name, "round_bytes": round_bytes, "waves_per_cu": waves, "payload_steps_per_round": steps_per_round,
            "per_round": {k: round(v, 1) for k, v in per.items()}, "lds_cycles_per_round": round(lds_cyc, 1),
            "valu_per_byte": round(per["valu"] / round_bytes, 4), "lds_cycles_per_byte": round(lds_cyc / round_bytes, 4),
            "rounds_per_wave": round(rounds_per_wave, 2), "valu_limit_us": round(valu_us, 1),
            "lds_limit_us": round(lds_us, 1), "_chain_trips_per_wave": rounds_per_wave * per["depth"],
            "u_lds_needed_for_38us": round(lds_us * U_L / (38.0 - PROLOGUE_US), 2)}


def main():
    pay_per_8k = 8192 / (PAYLOAD / NPAY)       # ~60 payloads per 8 KiB of stream
    # shipped k_stream: 8 KiB rounds, 8 waves; lane = 128 B = four 32-B blocks
    s8 = {"stage": phase(b128=16, valu=24),                     # 8 ds_write_b128 + 8 ds_read_b128, load addresses
          "chain": phase(n_apply=28 + 4 + 3, depth=-(28 + 4 + 3) + 8 + 3),  # 4 blocks x 7 steps in parallel, fold, Horner
          "scan": phase(n_nib=7),                               # shift(G, 128 B) + 6 Kogge-Stone levels
          "anchors": phase(n_apply=3, b32=4),
          "meta": phase(valu=40, b32=4),                        # decode + bookkeeping per round
          "payload": phase(n_apply=8, n_nib=4, valu=30, b32=8, b128=2, depth=2)}  # st_feed (<= 7 + 1), 4 length digits
    steps8 = pay_per_8k / 64 * 1.2                              # ~1.1 steps (a window over two groups)
    a = design("k_stream shipped (8 KiB rounds, 8 waves)", 8192, 8, s8, steps8)
    # 16-wave variant: 4 KiB rounds (lane = 64 B = two 32-B blocks), payload phase once per two rounds
    s16 = {"stage": phase(b128=8, valu=12),
           "chain": phase(n_apply=14 + 2 + 1, depth=-(14 + 2 + 1) + 8 + 1),
           "scan": phase(n_nib=7),
           "anchors": phase(n_apply=1, b32=2),
           "meta": phase(valu=25, b32=2),
           "payload": phase(n_apply=8, n_nib=4, valu=30, b32=8, b128=2, depth=2)}
    b = design("k_stream 16 waves, 4 KiB rounds, payloads of two rounds per step", 4096, 16, s16, steps8 / 2)
    # calibrate L on the shipped kernel: chain limit = measured - prologue
    L8 = (MEASURED["k_stream8"] - PROLOGUE_US) * 1e-6 * CLK / a["_chain_trips_per_wave"]
    # the LDS queue's load (issue cycles per unit time) at the predicted rate scales L at 16 waves
    res = []
    for d, L in ((a, L8), (b, None)):
        if L is None:  # iterate: the queueing delay grows with the LDS load the faster rate puts on it
            t = 40.0
            for _ in range(50):
                load_ratio = (b["lds_limit_us"] * U_L / t) / (a["lds_limit_us"] * U_L / MEASURED["k_stream8"])
                L = max(130.0, L8 * load_ratio)
                chain_us = d["_chain_trips_per_wave"] * L / CLK * 1e6
                t = PROLOGUE_US + max(d["valu_limit_us"], d["lds_limit_us"], chain_us)
        chain_us = d["_chain_trips_per_wave"] * L / CLK * 1e6
        d["lds_round_trip_cycles"] = round(L, 0)
        d["chain_limit_us"] = round(chain_us, 1)
        d["predicted_us"] = round(PROLOGUE_US + max(d["valu_limit_us"], d["lds_limit_us"], chain_us), 1)
        d["predicted_frac"] = round(READ / (d["predicted_us"] * 1e-6) / 8e12, 3)
        d["binding"] = max((("valu", d["valu_limit_us"]), ("lds", d["lds_limit_us"]), ("chain", chain_us)),
                           key=lambda x: x[1])[0]
        for k in [k for k in d if k.startswith("_")]:
            d.pop(k)
        res.append(d)
    # the best case for the new design: LDS round trips no slower than the unloaded latency
    chain_best = res[1]["chain_limit_us"] * 130.0 / res[1]["lds_round_trip_cycles"]
    best_us = PROLOGUE_US + max(res[1]["valu_limit_us"], res[1]["lds_limit_us"], chain_best)
    decision = "not built" if res[1]["predicted_us"] > 38.0 else "build"
    print(json.dumps({
        "what": "C5 cost model: 16-wave k_stream with two-round payload batching (VERDICT r05 item 6)",
        "workload": {"payload_bytes": PAYLOAD, "read_bytes": READ, "packets": NPAY},
        "calibration": {"u_valu": U_V, "u_lds": U_L, "prologue_us": PROLOGUE_US, "measured_us": MEASURED},
        "designs": res,
        "best_case_unloaded_lds_us": round(best_us, 1),
        "piece_kernel_shipped_us": MEASURED["k_pieces"],
        "threshold_us": 38.0, "decision": decision,
        "why": "the 16-wave design halves the bytes per scan (7 nibble operators per 4 KiB instead of per 8 KiB), so "
               "its VALU and LDS work per byte rise; at the LDS utilisation any mixed-length kernel here reached "
               "(0.48) its LDS limit alone is above the threshold, and its dependent-round-trip chain only meets it "
               "if LDS latency stays at the unloaded value while the LDS queue carries more load than today"}, indent=1))


if __name__ == "__main__":
    main()
