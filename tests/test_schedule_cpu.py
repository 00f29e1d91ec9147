"""The table of schedule-only options (tests/schedule_knobs.py) stays complete and inside the library's ranges: every key hr_set_option and
hr_set_debug_option know — the PRODUCT_OPTIONS and DEBUG_OPTIONS rows and the keys handled by explicit code — is read out of hr_api.hip and must be
either a row of the table (tests/test_schedule_gpu.py sweeps it) or an entry of OTHER_OPTIONS, which says why not and names the test that covers
it.  A new option fails here until someone decides which of the two it belongs to."""
import os
import re

import pytest

import schedule_knobs as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = os.path.join(ROOT, "hanamaru-renderer_amd", "csrc", "hr_api.hip")
NUM = r"(-?[0-9.]+(?:e[0-9]+)?|1 << 16)"
ROW = re.compile(r'\{"(\w+)", &hr_ctx::(\w+), %s, %s, %s, "' % (NUM, NUM, NUM))


def _number(s):
    return float(1 << 16) if s == "1 << 16" else float(s)


def _tables():
    """{"PRODUCT_OPTIONS": {key: (field, lo, hi, step)}, "DEBUG_OPTIONS": ..}"""
    src = open(API).read()
    out = {}
    for name in ("PRODUCT_OPTIONS", "DEBUG_OPTIONS"):
        body = re.search(r"static const OptionRow %s\[\] = \{\n(.*?)\n\};" % name, src, re.S).group(1)
        rows = {m.group(1): (m.group(2), _number(m.group(3)), _number(m.group(4)), _number(m.group(5))) for m in ROW.finditer(body)}
        assert len(rows) == len(re.findall(r'^\s*\{"', body, re.M)), "a row of %s does not parse" % name
        out[name] = rows
    return out


def _explicit_keys():
    """the keys behind `k == "..."` in hr_set_option / hr_set_debug_option: {key: "set_option" | "set_debug_option"}"""
    src = open(API).read()
    out = {}
    for fn, setter in (("hr_set_option", "set_option"), ("hr_set_debug_option", "set_debug_option")):
        body = re.search(r"\nint %s\(hr_ctx \*c, const char \*key, double value\) \{\n(.*?)\n\}\n" % fn, src, re.S).group(1)
        for key in re.findall(r'k == "(\w+)"', body):
            out.setdefault(key, setter)
    return out


def _all_keys():
    t = _tables()
    keys = {k: "set_option" for k in t["PRODUCT_OPTIONS"]}
    keys.update({k: "set_debug_option" for k in t["DEBUG_OPTIONS"]})
    for k, setter in _explicit_keys().items():
        keys.setdefault(k, setter)
    return keys


# the keys behind explicit code: the hr_ctx field each one sets (max_tail_gib is kept in bytes: `20ull << 30`)
EXPLICIT_FIELDS = {"moments": "moments_on", "sample_counts": "counts_on", "robust_buckets": "robust_k", "guide_bounces": "guide_bounces",
                   "russian_roulette": "rr_start", "seed_mode": "seed_mode", "nee_cull": "nee_cull", "split_ratio": "split_ratio",
                   "max_tail_gib": "max_tail_bytes"}


def _constant(name):
    """the value of `static const <type> name = <number>;` somewhere under csrc/"""
    csrc = os.path.dirname(API)
    found = [m.group(1) for f in sorted(os.listdir(csrc)) if f.endswith(".h")
             for m in re.finditer(r"^static const \w+ %s = (\d+);" % name, open(os.path.join(csrc, f)).read(), re.M)]
    assert len(found) == 1, (name, found)
    return int(found[0])


def _initialiser(ctx, field):
    """the default of hr_ctx::field as a number: an integer, false / true, -1.0, `20ull << 30` (returned in GiB) or a named constant"""
    m = re.search(r"\b%s = ([^,;]+)[,;]" % field, ctx)
    assert m, "no initialiser of hr_ctx::%s" % field
    text = m.group(1).strip()
    if text in ("false", "true"):
        return int(text == "true")
    if re.fullmatch(r"-?\d+", text):
        return int(text)
    if re.fullmatch(r"-?\d+\.\d+", text):
        return float(text)
    if re.fullmatch(r"\d+ull << 30", text):
        return int(text.split("ull")[0])
    if re.fullmatch(r"[\w:]+", text):
        return _constant(text.split("::")[-1])
    raise AssertionError("the initialiser of hr_ctx::%s does not parse: %r" % (field, text))


def test_the_parser_sees_the_option_tables():
    t = _tables()
    assert {"counters", "batch", "trace_boost", "precise_shading"} <= set(t["PRODUCT_OPTIONS"])
    assert {"kchunk", "tail_div", "trace_grid", "trace_budget", "wf_trav_wgs", "debug_skip"} <= set(t["DEBUG_OPTIONS"])
    assert {"moments", "sample_counts", "russian_roulette", "seed_mode", "nee_cull"} <= set(_explicit_keys())
    assert t["DEBUG_OPTIONS"]["kchunk"] == ("kchunk", 0.0, 64.0, 0.0) and t["PRODUCT_OPTIONS"]["trace_boost"] == ("trace_boost", -1.0, 4.0, 1.0)
    ctx = "bool a = false, b = true;\n    double r = -1.0;\n    uint64_t t = 20ull << 30;\n    uint32_t p = hr::lbvh::PLOC_TOP_CLUSTERS;\n    int n = -1;"
    assert [_initialiser(ctx, f) for f in "abrtn"] == [0, 1, -1.0, 20, -1] and isinstance(_initialiser(ctx, "r"), float)
    assert _initialiser(ctx, "p") == _constant("PLOC_TOP_CLUSTERS") == 8192
    with pytest.raises(AssertionError):
        _initialiser("int x = some(call);", "x")
    with pytest.raises(AssertionError):
        _initialiser(ctx, "missing")


def test_every_option_is_in_the_table_or_in_the_list_of_the_others():
    keys = _all_keys()
    both = set(K.KNOBS) & set(K.OTHER_OPTIONS)
    assert not both, "in the table AND in OTHER_OPTIONS: %s" % sorted(both)
    missing = sorted(set(keys) - set(K.KNOBS) - set(K.OTHER_OPTIONS))
    assert not missing, "options neither in schedule_knobs.KNOBS (schedule-only: swept bit for bit) nor in OTHER_OPTIONS (with the test that covers them): %s" % missing
    gone = sorted((set(K.KNOBS) | set(K.OTHER_OPTIONS)) - set(keys))
    assert not gone, "schedule_knobs names options hr_api.hip does not have: %s" % gone
    for key, (kind, covered_by, _, _) in K.OTHER_OPTIONS.items():
        assert kind in ("axis", "image", "variant") and "test" in covered_by, key
        for path in re.findall(r"(?:tests/)?(test_\w+\.py)", covered_by):
            assert os.path.exists(os.path.join(ROOT, "tests", path)), (key, path)
        for path, name in re.findall(r"(test_\w+\.py)::(test_\w+)", covered_by):
            assert re.search(r"^def %s\(" % name, open(os.path.join(ROOT, "tests", path)).read(), re.M), (key, path, name)


def test_setters_and_defaults_are_the_librarys():
    keys, t = _all_keys(), _tables()
    src = open(API).read()
    ctx = re.search(r"\nstruct hr_ctx \{\n(.*?)\n\};", src, re.S).group(1)
    assert set(K.ALL_DEFAULTS) == set(K.SETTERS) == set(keys)
    explicit = _explicit_keys()
    for key, default in K.ALL_DEFAULTS.items():
        assert keys[key] == K.SETTERS[key], key
        rows = t["PRODUCT_OPTIONS" if K.SETTERS[key] == "set_option" else "DEBUG_OPTIONS"]
        if key == "rng_window":      # no field: the one value the explicit code accepts
            assert key in explicit and default == _constant("ISAAC_TAIL"), key
            continue
        assert (key in rows) != (key in EXPLICIT_FIELDS), key
        got = _initialiser(ctx, rows[key][0] if key in rows else EXPLICIT_FIELDS[key])
        assert got == default and type(got) is type(default), (key, got, default)
    for k in K.KNOBS.values():
        assert keys[k.key] == k.setter, k.key
        row = t["PRODUCT_OPTIONS" if k.setter == "set_option" else "DEBUG_OPTIONS"][k.key]
        m = re.search(r"\b%s = (-?\d+)\b" % row[0], ctx)
        assert m, "no initialiser of hr_ctx::%s" % row[0]
        assert int(m.group(1)) == k.default, (k.key, m.group(1), k.default)
        assert set(k.pipelines) <= {K.MEGA, K.SPLIT} and k.pipelines and set(k.reduced) <= set(k.values), k.key
    assert list(K.DEFAULTS) == list(K.KNOBS)


def _in_range(row, v):
    _, lo, hi, step = row
    if lo > hi:       # (a row without a range)
        return True
    return lo <= v <= hi and (step <= 0 or (v - lo) % step == 0)


def test_every_table_value_lies_in_the_range_of_its_option_row():
    t = _tables()
    for k in K.KNOBS.values():
        row = t["PRODUCT_OPTIONS" if k.setter == "set_option" else "DEBUG_OPTIONS"][k.key]
        assert row[1] <= row[2], "%s: a schedule knob without a range" % k.key
        for v in tuple(k.values) + (k.default,):
            assert _in_range(row, v), (k.key, v, row)
    for name, setting in K.COMBINED.items():
        assert set(setting) == set(K.KNOBS), name
        for key, v in setting.items():
            k = K.KNOBS[key]
            assert _in_range(t["PRODUCT_OPTIONS" if k.setter == "set_option" else "DEBUG_OPTIONS"][key], v), (name, key, v)


def test_the_edge_values_stay_in_the_table():
    """the values at which the unit, grid and budget arithmetic changes its path (the reasons stand beside the rows): none is dropped by accident"""
    want = {"kchunk": {1, 2, 3, 5, 64}, "tail_div": {0, 1, 2, 16, 1000000}, "trace_grid": {1, 3, 1000000}, "trace_wgs": {1, 8},
            "trace_budget": {1, 2, 15, 16, 17, 31, 32, 33, 1000000}, "adv_den": {1, 64}, "leaf_den": {1, 64}, "node_unroll": {1},
            "seed_prio": {0, 1, 2, 3}, "init_prio": {0, 1, 2, 3}, "trace_boost": {0, 1, 2, 3, 4}, "wf_adv_den": {0, 1, 64},
            "wf_trav_wgs": {1, 16}, "wf_shade_wgs": {1, 16}}
    for key, values in want.items():
        assert values <= set(K.KNOBS[key].values), key
    assert set(K.KNOBS["trace_budget"].pipelines) == {K.MEGA, K.SPLIT}
    reduced = {"kchunk": {1, 5}, "tail_div": {1, 1000000}, "trace_grid": {1}, "trace_budget": {1, 17}, "wf_trav_wgs": {1}, "wf_shade_wgs": {1}}
    for k in K.KNOBS.values():
        assert set(k.reduced) == reduced.get(k.key, set()), k.key


@pytest.mark.parametrize("pipeline", [K.MEGA, K.SPLIT])
def test_settings_cover_the_rows_of_the_pipeline(pipeline):
    full, reduced = K.settings(pipeline, True), K.settings(pipeline, False)
    for k in K.KNOBS.values():
        got = {s[k.key] for _, s in full if list(s) == [k.key]}
        assert got == ({v for v in k.values if v != k.default} if pipeline in k.pipelines else set()), k.key
    assert [name for name, _ in full[-2:]] == ["smallest", "largest"] == [name for name, _ in reduced[-2:]]
    assert len({name for name, _ in full}) == len(full) and {name for name, _ in reduced} <= {name for name, _ in full}
    assert all(set(s) <= set(K.UNIT_KNOBS) or len(s) > 1 for _, s in K.settings(pipeline, True, keys=K.UNIT_KNOBS))
    assert all(len(s) == 1 and set(s) <= set(K.PATH_LOG_KNOBS) for _, s in K.settings(pipeline, True, keys=K.PATH_LOG_KNOBS, combined=False))
