"""Tables that bre_set_materials_ex, bre_check_material_table_ex and bre_device_check kind 14 refuse because of a mix,
each with words of the message (test infrastructure), shared by tests/test_mix_refpy.py (no device) and
tests/test_mix_gpu.py (a live context).  The refused material is always the table's last entry.
"""


def _bad_mix(sm, **fields):
    m = sm.mix(0, 0, 0.5)
    for k, v in fields.items():
        if k == "reserved2":
            m.reserved[2] = v
        elif k == "child0":
            m.reserved[0] = v
        elif k in ("kr", "kt", "ks", "ceta", "ck", "amount"):
            setattr(m, k, sm._rgb(v))
        else:
            setattr(m, k, v)
    return m


def bad_records(sm):
    """(a mix record that is refused on its own, words of why)."""
    nan = float("nan")
    return [(_bad_mix(sm, amount=(0.5, nan, 0.5)), "a non-finite amount (mix)"),
            (_bad_mix(sm, amount=(float("inf"), 0.5, 0.5)), "a non-finite amount (mix)"),
            (_bad_mix(sm, child0=-1), "a negative child index -1 (mix: mix_child[0])"),
            (_bad_mix(sm, reserved2=1), "a non-zero reserved[2] (mix"),
            (_bad_mix(sm, kr=0.5), "a non-zero Kr, which a mix does not read"),
            (_bad_mix(sm, kt=(0, 0, 0.1)), "a non-zero Kt, which a mix does not read"),
            (_bad_mix(sm, eta=1.5), "a non-zero eta, which a mix does not read"),
            (_bad_mix(sm, ks=0.25), "a non-zero Ks, which a mix does not read"),
            (_bad_mix(sm, ceta=(0, nan, 0)), "a non-finite metal eta, which a mix does not read"),
            (_bad_mix(sm, ck=1.0), "a non-zero k, which a mix does not read"),
            (_bad_mix(sm, roughness=0.1), "a non-zero roughness, which a mix does not read"),
            (_bad_mix(sm, uroughness=0.1), "a non-zero uroughness, which a mix does not read"),
            (_bad_mix(sm, vroughness=0.1), "a non-zero vroughness, which a mix does not read"),
            (_bad_mix(sm, sigma=20.0), "a non-zero sigma, which a mix does not read"),
            (_bad_mix(sm, remap=1), "a non-zero remap, which a mix does not read")]


def bad_tables(sm):
    """(a table whose last entry is refused, words of why): every record above behind a matte, then the rules between
    records."""
    five = sm.uber((0.4, 0.3, 0.2), (0.3, 0.4, 0.5), (0.5, 0.5, 0.6), (0.7, 0.6, 0.5), 0.1, 0.0, 0.0, 1.5, (0.6, 0.7, 0.8))
    out = [([sm.matte(0.5), m], "material 1 has " + word) for m, word in bad_records(sm)]
    out.append(([sm.matte(0.5), sm.mix(0, 1)], "material 1 has child 1 (mix_child[1]) that does not come before it"))
    out.append(([sm.matte(0.5), sm.mix(7, 0)], "material 1 has child 7 (mix_child[0]) that does not come before it"))
    deep = [sm.matte(0.5)] + [sm.mix(k, 0) for k in range(5)]
    out.append((deep, "material 5 has a nest 5 mixes deep (at most BRE_MAX_MIX_DEPTH = 4)"))
    out.append(([five, sm.translucent(), sm.mix(0, 1)],
                "material 2 has 9 BxDFs after expansion (at most BRE_MAX_BXDFS = 8"))
    return out


def good_tables(sm):
    """Tables at the limits, which are accepted: four mixes deep, eight BxDFs, a black amount, a child used twice."""
    five = sm.uber((0.4, 0.3, 0.2), (0.3, 0.4, 0.5), (0.5, 0.5, 0.6), (0.7, 0.6, 0.5), 0.1, 0.0, 0.0, 1.5, (0.6, 0.7, 0.8))
    return [[sm.matte(0.5)] + [sm.mix(k, 0) for k in range(4)],
            [five, sm.translucent((0.5, 0.4, 0.3), 0.0, 0.6, 0.4), sm.widen(sm.mirror(0.9)), sm.mix(0, 1), sm.mix(3, 2)],
            [sm.matte(0.5), sm.mix(0, 0, 0.0)], [sm.matte(0.5), sm.mix(0, 0, (2.0, -1.0, 0.5))]]
