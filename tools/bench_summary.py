import json,sys
d=json.load(open(sys.argv[1]))
roof = d.get("roofline")      # only a bench.py --full line carries it
print("steps/s", round(d["value"],1), "ms/step", round(d["ms_per_step"],5), *(("frac", round(roof["frac"],4)) if roof else ()))
if roof:
    for r in roof["launches"]: print(f'{r["launch"]:32s} {r["avg_us"]:7.2f}')
    print("eager_step_us", roof["eager_step_us"])
