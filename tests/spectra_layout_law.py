"""The spectra block of a slot (include/wayne_hip.h, "The spectra block"), restated: which regions it holds for a set of
options, where each begins and how long it is.  All float64 but n_rejected (uint32); only behind those 4-byte counts can
the next region need padding to a multiple of 8 bytes."""

ORDER = ("spectra", "sky", "n_rejected", "channels", "spectra_var", "sky_var", "channels_var", "optimal", "optimal_var",
         "channels_opt", "channels_opt_var")


def sizes(S, R, crrej=False, C=0, variance=False, optimal=False, optimal_channels=False):
    """{region: bytes} of the regions that are on, in the block's order."""
    assert not optimal or variance, "the optimal products need the variances"
    assert not optimal_channels or (optimal and C), "the optimal channels need the channels and the optimal products"
    n = R + 1
    on = {"spectra": n * S * 8, "sky": n * 8}
    if crrej:
        on["n_rejected"] = n * 4
    if C:
        on["channels"] = n * C * 8
    if variance:
        on.update(spectra_var=n * S * 8, sky_var=n * 8)
        if C:
            on["channels_var"] = n * C * 8
    if optimal:
        on.update(optimal=n * S * 8, optimal_var=n * S * 8)
    if optimal_channels:
        on.update(channels_opt=n * C * 8, channels_opt_var=n * C * 8)
    return {k: on[k] for k in ORDER if k in on}


def layout(S, R, **options):
    """({region: byte offset} of the regions that are on, the block's bytes)."""
    on = sizes(S, R, **options)
    at, off = 0, {}
    for name, size in on.items():
        off[name] = at
        at += size
        if name == "n_rejected" and name != list(on)[-1]:
            at += -at % 8                                            # the region behind the counts starts on 8 bytes
    return off, at


def combinations():
    """Every legal combination of the five switches, as keyword dictionaries without C (with_c: channels are on)."""
    for crrej in (False, True):
        for with_c in (False, True):
            for variance in (False, True):
                for optimal in ((False, True) if variance else (False,)):
                    for optch in ((False, True) if (optimal and with_c) else (False,)):
                        yield dict(crrej=crrej, variance=variance, optimal=optimal, optimal_channels=optch), with_c
