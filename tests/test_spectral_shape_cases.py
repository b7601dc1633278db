"""CPU side of the shape sweep of the device spectral synthesis (tests/spectral_shape_cases.py, tests/test_gpu_spectral_shapes.py):
the conditions that make the sweep's flat bar of 1e-12 x scale a fair one, and the coverage of the geometry restatement."""
import numpy as np

import spectral_shape_cases as sc


def test_restated_table_decisions():
    """The restatement's expectations for the 64 tables of the sweep; tests/test_gpu_spectral_shapes.py asserts the same decisions
    against the device (refusals, strip_active)."""
    plans = {k: sc.table_plan(k) for k in sc.ALL_TABLES}
    refused = sorted(k for k, p in plans.items() if not p["admissible"])
    wide = [k for k, p in plans.items() if p["wide"]]
    strip = [k for k, p in plans.items() if p["strip"]]
    on = sum(sum(p["split2"]) for p in plans.values())
    off = sum(len(p["shapes"]) - sum(p["split2"]) for p in plans.values() if p["strip"])
    print(f"\n    admissible {64 - len(refused)} of 64 (refused {refused}), wide {len(wide)}, strip-eligible {len(strip)}: "
          f"split2 on {on} shapes, off {off}")
    assert refused == [(6, 7), (7, 5), (7, 6), (7, 7)]
    assert (len(wide), len(strip), on, off) == (15, 36, 2232, 72)
    assert all(sc.set_blocks_ok(p["sizes"]) for p in plans.values())          # every refusal is the proposal kernel's
    for name in sc.EXTRA:
        p = sc.table_plan(name)
        assert p["admissible"] and not p["strip"] and len(p["shapes"]) == 64, name


def test_every_geometry_class_is_covered():
    """Each class of shapes at which the folds, the padding and the clamped last K step differ has cases in the sweep.  The
    classes are those of spectral_shape_cases.classes; the 'static' handles run the split stage 2 where the restatement says so."""
    keys = sc.ALL_TABLES + list(sc.EXTRA)
    static, bare = sc.count_classes(keys, True), sc.count_classes(keys, False)
    print("\n    class counts (static handles): " + ", ".join(f"{c} {static.get(c, 0)}" for c in sc.REQUIRED_CLASSES))
    print("    bare handles: split2 on " + str(bare.get("strip_split2_on", 0)) + ", shapes " + str(bare["bh%4=0"] + bare["bh%4=2"]))
    missing = [c for c in sc.REQUIRED_CLASSES if static.get(c, 0) == 0]
    assert not missing, missing
    assert not any(c.startswith("s2_last") or c.startswith("strip_") for c in bare)       # bare handles: direct stage 2 everywhere
    assert bare["bh%4=0"] + bare["bh%4=2"] == 60 * 64 + 128
    # more than 8 tiles along a side is out of reach of lengths <= 128: the two EXTRA tables alone hold that class
    assert sc.count_classes(sc.ALL_TABLES).get("tiles_per_side>8", 0) == 0 and static["tiles_per_side>8"] == 128


def test_the_flat_bar_is_fair():
    """Measured (this test prints both figures):
      * |mean| / (std + 1e-12) of the raw ifft2 field, the factor by which the standardisation amplifies the DFT's rounding: at
        most 18 (Matern, over 4224 shapes x 3 models); asserted <= 100.
      * the oracle against a long-double DFT of the same coefficients on the fixed subsample (546 cases): at most 1.3e-14 x scale;
        asserted <= 1e-13 x scale.  The device bar of 1e-12 x scale sits ~80 x above the reference's own rounding."""
    worst = (0.0, None)
    shapes = [s for k in sc.ALL_TABLES + list(sc.EXTRA) for s in sc.table_plan(k)["shapes"]]
    cache = {}
    for bh, bw in shapes:
        d = cache[(bh, bw)] = sc.draws(bh, bw)
        for model, _ in sc.MODELS:
            f = sc.raw_field(d, model, (bh, bw))
            r = abs(f.mean()) / (f.std() + 1e-12)
            if r > worst[0]:
                worst = (r, (bh, bw, model))
    print(f"\n    {len(shapes)} shapes x 3 models: worst |mean| / std of the raw field {worst[0]:.2f} at {worst[1]}")
    assert worst[0] <= 100.0
    sub = sc.subsample()
    dev = (0.0, None)
    for bh, bw, m in sub:
        model, nugget = sc.MODELS[m]
        d = cache[(bh, bw)]
        e = sc.expected(d, model, nugget, (bh, bw))
        ld = sc.longdouble_field(d, model, nugget, (bh, bw))
        err = float(np.abs(e.astype(np.longdouble) - ld).max()) / d["scale"]
        if err > dev[0]:
            dev = (err, (bh, bw, model))
    print(f"    oracle against the long-double DFT on {len(sub)} cases: worst {dev[0]:.2e} x scale at {dev[1]}")
    assert len(sub) >= 540 and dev[0] <= 1e-13
