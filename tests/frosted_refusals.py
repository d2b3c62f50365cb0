"""The records bre_set_materials_ex refuses and accepts for the rough glass, uber, translucent and substrate types
(test infrastructure): (record, a word of the message it must be refused with)."""


def bad_records(sm):
    nan, inf = float("nan"), float("inf")

    def edit(m, **kw):
        for k, v in kw.items():
            if k.startswith("reserved"):
                m.reserved[int(k[-1])] = v
            elif isinstance(v, tuple):
                setattr(m, k, sm.F3(*v))
            else:
                setattr(m, k, v)
        return m

    return [
        # a non-finite parameter of the record's type
        (sm.rough_glass(nan, 1.0, 1.5, 0.1, 0.1), "non-finite Kr"), (sm.rough_glass(1.0, inf, 1.5, 0.1, 0.1), "non-finite Kt"),
        (sm.rough_glass(1.0, 1.0, 1.5, nan, 0.1), "non-finite uroughness"), (sm.uber(kd=nan), "non-finite Kd"),
        (sm.uber(opacity=inf), "non-finite opacity"), (sm.uber(roughness=nan), "non-finite roughness"),
        (sm.translucent(reflect=nan), "non-finite reflect"), (sm.translucent(roughness=inf), "non-finite roughness"),
        (sm.substrate(ks=nan), "non-finite Ks"), (sm.substrate(vroughness=nan), "non-finite vroughness"),
        # eta
        (sm.rough_glass(1.0, 1.0, 0.0, 0.1, 0.1), "eta"), (sm.rough_glass(1.0, 1.0, -1.5, 0.1, 0.1), "rough glass"),
        (sm.uber(eta=nan), "eta"), (sm.uber(eta=0.0), "uber"),
        # remap
        (edit(sm.substrate(), remap=2), "remap"), (edit(sm.uber(), remap=-1), "remap"),
        # an alpha that is not > 0 after the material's own mapping
        (sm.rough_glass(1.0, 1.0, 1.5, 0.0, 0.2, remap=False), "alpha"), (sm.rough_glass(1.0, 1.0, 1.5, 0.2, -0.1, remap=False), "alpha"),
        (sm.uber(roughness=0.0, remap=False), "alpha"), (sm.uber(roughness=0.1, vroughness=-0.2, remap=False), "alpha"),
        (sm.translucent(roughness=0.0, remap=False), "alpha"), (sm.substrate(uroughness=0.0, remap=False), "alpha"),
        # both roughnesses 0: that is smooth glass
        (sm.rough_glass(1.0, 1.0, 1.5, 0.0, 0.0), "BRE_MATERIAL_GLASS"),
        (sm.rough_glass(1.0, 1.0, 1.5, 0.0, 0.0, remap=False), "BRE_MATERIAL_GLASS"),
        # a field the type does not read
        (edit(sm.rough_glass(1.0, 1.0, 1.5, 0.1, 0.1), kd=(0.1, 0.0, 0.0)), "Kd"),
        (edit(sm.rough_glass(1.0, 1.0, 1.5, 0.1, 0.1), roughness=0.1), "roughness"),
        (edit(sm.rough_glass(1.0, 1.0, 1.5, 0.1, 0.1), opacity=(1.0, 1.0, 1.0)), "opacity"),
        (edit(sm.translucent(), opacity=(0.0, 0.5, 0.0)), "opacity"), (edit(sm.substrate(), ceta=(0.0, 0.0, 1.0)), "opacity"),
        (edit(sm.translucent(), eta=1.5), "eta"), (edit(sm.translucent(), uroughness=0.1), "uroughness"),
        (edit(sm.substrate(), kr=(0.5, 0.5, 0.5)), "Kr"), (edit(sm.substrate(), roughness=0.1), "roughness"),
        (edit(sm.uber(), sigma=10.0), "sigma"), (edit(sm.uber(), ck=(0.0, 1.0, 0.0)), "k"),
        (edit(sm.substrate(), eta=1.5), "eta"),
        # the reserved words stay zero for every type
        (edit(sm.uber(), reserved0=1), "reserved"), (edit(sm.rough_glass(1.0, 1.0, 1.5, 0.1, 0.1), reserved2=1), "reserved"),
    ]


def good_records(sm):
    """Accepted: colours outside [0, 1] are clamped; with remaproughness one roughness of a rough glass may be 0."""
    return [sm.rough_glass(1.5, -0.5, 1.5, 0.0, 0.2, remap=True), sm.uber(1.5, -1.0, 2.0, 0.5, opacity=(1.5, 0.5, -1.0)),
            sm.translucent(2.0, 0.5, 1.5, -0.5), sm.substrate(1.5, 1.5, 0.0, 0.0, remap=True),
            sm.uber(roughness=0.0, remap=True)]
