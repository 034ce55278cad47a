#!/usr/bin/env python3
"""A radiative-convective column: RRTMG shortwave + longwave and the slab surface under Adams-Bashforth, followed at every step by
the dry convective adjustment -- the arrangement of the reference's examples/column_code_with_slab.py with
`from climt_amd import ...`: one column of 30 levels, dt = 10 min, a 5 m ocean mixed layer at 300 K under a fixed sun.

The reference's example also couples the column to the surface with SimplePhysics (--simple-physics below) and carries
EmanuelConvection in the time stepper's list (--moist-convection below): by default the atmosphere feels the surface through the
radiation alone and stays dry.  So that the adjustment has work from
the first step, the column starts on a lapse rate steeper than the dry adiabat (T ~ p^0.32) instead of the reference's
isothermal 290 K.

    python examples/radiative_convective.py [--steps 60] [--device-resident] [--boundary-layer | --simple-physics] [--moist-convection]
                                            [--gray-longwave | --cork-longwave TABLE] [--cork-shortwave TABLE] [--grid-scale-condensation] [--sea-ice]
                                            [--land-surface bucket|second_best]

--boundary-layer closes that gap: SimpleBoundaryLayer (bulk surface fluxes, implicit diffusion of T, q, u, v) steps after the time
stepper and before the adjustment, and its two flux diagnostics go into the state, so the slab feels them from the next step
on.  The state then carries a light wind and a surface humidity.  Without the flag the run is what it was.

--simple-physics is the reference's own coupling: SimplePhysics (large-scale condensation, surface fluxes on the lowest layer,
boundary-layer mixing) steps after the time stepper and before the adjustment, as in the reference's column_code_with_slab.py,
and its diagnostics -- the two surface fluxes and the stratiform precipitation -- go into the state.  The state then carries a
light wind, and the column starts moister with a supersaturated layer, so that it rains from the first step.  Exclusive with
--boundary-layer (both would exchange with the surface).  Without the flag the run is what it was.

--moist-convection puts EmanuelConvection into the AdamsBashforth list, as the reference's example has it
(AdamsBashforth([rad_sw, rad_lw, slab, convection])): what the column holds of water condenses and rains out, the cloud-base mass
flux is carried from step to step, and the precipitation joins the report.  The column then starts moister (80 % of saturation
near the surface).  Without the flag the run is what it was.

--gray-longwave replaces the RRTMG longwave with the gray one of the Frierson set-up: GrayLongwaveRadiation with the optical depth
of Frierson06LongwaveOpticalDepth formed inside the sweep (the fused call; the depth joins the diagnostics).  The shortwave stays
RRTMG's.  Without the flag the run is what it was.

--cork-longwave TABLE replaces the RRTMG longwave with the table-driven correlated-k one: CorkLongwaveRadiation(optics="correlated_k",
table=TABLE), TABLE a k-table file (tests/golden/cork_table_earth4.npz say) or what else the component takes.  The state then
carries the emissivity and the cloud depth on the table's own bands; the per-band diagnostics join the others.  The shortwave
stays RRTMG's.  Exclusive with --gray-longwave.  Without the flag the run is what it was.

--cork-shortwave TABLE replaces the RRTMG shortwave with the correlated-k two-stream one: CorkShortwaveRadiation(optics=
"correlated_k", table=TABLE), TABLE a shortwave k-table file (tests/golden/cork_sw_table_sw_earth.npz say).  The state then carries
the three cloud arrays on the table's own bands.  Without the flag the run is what it was.

--grid-scale-condensation adds GridScaleCondensation, the moisture sink of that set-up, after the time stepper (and after the
boundary layer where there is one) and before the adjustment; its precipitation_amount goes into the state.  The column then
starts at 70 % of saturation with one supersaturated layer.  Exclusive with --simple-physics, which condenses itself.  Without
the flag the run is what it was.

--device-resident keeps the state in HBM (climt_amd.DeviceState + DeviceAdamsBashforth; the adjustment reads and rebinds the
resident temperature and humidity): same components, same numbers.  The longwave k-distribution tables of this build are
synthetic while the reference's data file is missing (the component says so).
"""
import argparse
import os
import sys
from datetime import timedelta

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from climt_amd import (AdamsBashforth, CorkLongwaveRadiation, CorkShortwaveRadiation, DryConvectiveAdjustment, EmanuelConvection, Frierson06LongwaveOpticalDepth, GrayLongwaveRadiation,  # noqa: E402
                       GridScaleCondensation, RRTMGLongwave, SeaIce, BucketHydrology, SecondBEST, RRTMGShortwave, SimpleBoundaryLayer, SimplePhysics, SlabSurface, get_default_state, get_grid)


def run(steps=60, device_resident=False, report=None, boundary_layer=False, moist_convection=False, simple_physics=False, gray_longwave=False,
        grid_scale_condensation=False, sea_ice=False, land_surface=None, cork_longwave=None, cork_shortwave=None):
    """-> (diagnostics of step 0, state after `steps` steps), both as host DataArrays.  `boundary_layer`: with SimpleBoundaryLayer
    between the time stepper and the adjustment; its diagnostics of step 0 are then among the first.  `moist_convection`: with
    EmanuelConvection in the time stepper's list.  `simple_physics`: with SimplePhysics in the place of the boundary layer.
    `gray_longwave`: the fused Frierson + gray longwave in the place of RRTMG's.  `grid_scale_condensation`: with
    GridScaleCondensation before the adjustment.  `sea_ice`: the surface is 2 m of sea ice under 0.1 m of snow and SeaIce steps
    the snow/ice column in front of the time stepper (and so of SlabSurface, which reads the flux SeaIce writes).  The order in
    which things run is the order of the loop below; `steppers` only tells get_default_state and DeviceState.from_host which
    inputs to serve.  On the first step no radiation has run yet, so SeaIce reads the default state's radiative fluxes: zeros.
    `land_surface`: "bucket" or "second_best" -- the surface is land, and BucketHydrology or SecondBEST steps it in the place
    where SeaIce steps the ice (exclusive with `sea_ice`); SlabSurface reads the surface fluxes it writes.  `cork_longwave`: a
    k-table -- the correlated-k longwave on it in the place of RRTMG's (exclusive with `gray_longwave`).  `cork_shortwave`: a shortwave
    k-table -- the correlated-k two-stream shortwave on it in the place of RRTMG's."""
    if cork_longwave is not None and gray_longwave:
        raise ValueError("cork_longwave and gray_longwave are exclusive: one longwave scheme")
    if land_surface not in (None, "bucket", "second_best"):
        raise ValueError("land_surface must be None, 'bucket' or 'second_best'")
    if land_surface and sea_ice:
        raise ValueError("land_surface and sea_ice are exclusive: one surface type per column")
    if boundary_layer and simple_physics:
        raise ValueError("boundary_layer and simple_physics are exclusive: both exchange heat, moisture and momentum with the surface")
    if grid_scale_condensation and simple_physics:
        raise ValueError("grid_scale_condensation and simple_physics are exclusive: both remove grid-scale supersaturation")
    rad_sw = RRTMGShortwave() if cork_shortwave is None else CorkShortwaveRadiation(optics="correlated_k", table=cork_shortwave)
    if cork_longwave is not None:
        rad_lw = CorkLongwaveRadiation(optics="correlated_k", table=cork_longwave)
    else:
        rad_lw = GrayLongwaveRadiation(optical_depth=Frierson06LongwaveOpticalDepth()) if gray_longwave else RRTMGLongwave(allow_synthetic_tables=True)
    slab = SlabSurface()
    dry_convection = DryConvectiveAdjustment()
    components = [rad_sw, rad_lw, slab]
    if moist_convection:
        components = components + [EmanuelConvection()]
    time_stepper = AdamsBashforth(components)
    timestep = timedelta(minutes=10)
    steppers = [dry_convection]
    if boundary_layer:
        simple_boundary_layer = SimpleBoundaryLayer()
        steppers = [simple_boundary_layer, dry_convection]
    if simple_physics:
        simple_boundary_layer = SimplePhysics()      # (steps where the boundary layer steps)
        steppers = [simple_boundary_layer, dry_convection]
    if grid_scale_condensation:
        condensation = GridScaleCondensation()
        steppers = steppers[:-1] + [condensation, dry_convection]

    if sea_ice:
        ice = SeaIce()
        steppers = [ice] + steppers

    if land_surface:
        land = BucketHydrology() if land_surface == "bucket" else SecondBEST()
        steppers = [land] + steppers

    grid = get_grid(nx=1, ny=1, nz=30)
    state = get_default_state(components + steppers, grid_state=grid)
    p = state["air_pressure"].values
    state["air_temperature"].values[:] = np.maximum(210.0, 300.0 * (p / p.max()) ** 0.32)
    state["specific_humidity"].values[:] = 0.012 * (p / p.max()) ** 3
    for name in ("surface_albedo_for_direct_shortwave", "surface_albedo_for_direct_near_infrared", "surface_albedo_for_diffuse_shortwave"):
        if name in state:      # (the correlated-k shortwave reads the direct shortwave albedo alone)
            state[name].values[:] = 0.4
    state["zenith_angle"].values[:] = np.pi / 2.5
    state["surface_temperature"].values[:] = 300.0
    state["ocean_mixed_layer_thickness"].values[:] = 5.0
    state["area_type"].values[:] = "sea"
    if sea_ice:
        state["area_type"].values[:] = "sea_ice"
        state["sea_ice_thickness"].values[:] = 2.0
        state["surface_snow_thickness"].values[:] = 0.1
        total = 2.1
        n = state["height_on_ice_interface_levels"].values.shape[0]
        state["height_on_ice_interface_levels"].values[:] = (total * np.arange(n) / (n - 1)).reshape((n,) + (1,) * (state["height_on_ice_interface_levels"].values.ndim - 1))
        state["snow_and_ice_temperature"].values[:] = 265.0
        state["surface_temperature"].values[:] = 265.0
    if land_surface:
        state["area_type"].values[:] = "land"
        state["eastward_wind"].values[:] = 5.0
        state["surface_temperature"].values[:] = 295.0
        if land_surface == "bucket":
            state["surface_specific_humidity"].values[:] = 0.016
            state["lwe_thickness_of_soil_moisture_content"].values[:] = 0.08
        else:
            n = state["height_on_soil_interface_levels"].values.shape[0]
            state["height_on_soil_interface_levels"].values[:] = (-0.25 * np.arange(n)[::-1]).reshape((n,) + (1,) * (state["height_on_soil_interface_levels"].values.ndim - 1))
            state["soil_temperature"].values[:] = 295.0
            state["soil_liquid_water_content"].values[:] = 0.25
            state["soil_ice_content"].values[:] = 0.0
    if moist_convection:
        t = state["air_temperature"].values
        es = 611.2 * np.exp(17.67 * (t - 273.15) / (t - 29.65))
        state["specific_humidity"].values[:] = 0.8 * 0.622 * es / (p - 0.378 * es) * (p / p.max()) ** 1.5
    if boundary_layer:
        state["eastward_wind"].values[:] = 5.0
        state["surface_specific_humidity"].values[:] = 0.018
    if simple_physics:
        t = state["air_temperature"].values
        qsat = 287.0 / 461.5 * 610.78 / p * np.exp(-2.5e6 / 461.5 * (1.0 / t - 1.0 / 273.16))
        state["specific_humidity"].values[:] = 0.7 * qsat
        state["specific_humidity"].values[3] = 1.05 * qsat[3]      # one supersaturated layer: stratiform rain from step 0
        state["eastward_wind"].values[:] = 5.0
    if grid_scale_condensation:
        t = state["air_temperature"].values
        es = 611.2 * np.exp(17.67 * (t - 273.15) / (t - 29.65))
        qsat = 287.0 / 461.5 * es / (p - (1.0 - 287.0 / 461.5) * es)
        state["specific_humidity"].values[:] = 0.7 * qsat
        state["specific_humidity"].values[3] = 1.05 * qsat[3]      # one supersaturated layer: condensation from step 0
    to_host = lambda s, names=None: {k: s[k] for k in (names or s)}
    if device_resident:
        import climt_amd
        # a quantity is resident in the units of the first component that asks for it: the cork components read pressures in any one
        # unit, RRTMG's wants mbar, so RRTMG's components ask first (without a cork component the order is what it was)
        cork = (CorkLongwaveRadiation, CorkShortwaveRadiation)
        state = climt_amd.DeviceState.from_host(state, sorted(components, key=lambda c: isinstance(c, cork)) + steppers)
        time_stepper = climt_amd.DeviceAdamsBashforth(components)
        to_host = lambda s, names=None: {k: s.download(k) for k in (names or s) if k != "time"}

    first = None
    for i in range(steps):
        if sea_ice or land_surface:
            diagnostics, new_state = (ice if sea_ice else land)(state, timestep)
            state.update(diagnostics)
            state.update(new_state)
            if i == 0:
                first_ice = to_host(state, list(diagnostics))

        diagnostics, state = time_stepper(state, timestep)      # (the reference's order: the new state, then the diagnostics into it)
        state.update(diagnostics)
        if i == 0:
            first = to_host(state, list(diagnostics))
            if sea_ice or land_surface:
                first.update(first_ice)

        if boundary_layer or simple_physics:
            diagnostics, new_state = simple_boundary_layer(state, timestep)
            state.update(diagnostics)
            state.update(new_state)
            if i == 0:
                first.update(to_host(state, list(diagnostics)))

        if grid_scale_condensation:
            diagnostics, new_state = condensation(state, timestep)
            state.update(diagnostics)
            state.update(new_state)
            if i == 0:
                first.update(to_host(state, list(diagnostics)))

        diagnostics, new_state = dry_convection(state, timestep)
        state.update(diagnostics)
        state.update(new_state)
        if i % 10 == 0 and report is not None:
            report(i, to_host(state))
    end = to_host(state)
    if device_resident:
        state.close()      # hands the shared context back in the mode it was found in
    return first, end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--device-resident", action="store_true")
    surface = ap.add_mutually_exclusive_group()
    surface.add_argument("--boundary-layer", action="store_true")
    surface.add_argument("--simple-physics", action="store_true")
    ap.add_argument("--moist-convection", action="store_true")
    longwave = ap.add_mutually_exclusive_group()
    longwave.add_argument("--gray-longwave", action="store_true")
    longwave.add_argument("--cork-longwave", metavar="TABLE", default=None)
    ap.add_argument("--cork-shortwave", metavar="TABLE", default=None)
    ap.add_argument("--grid-scale-condensation", action="store_true")
    ap.add_argument("--sea-ice", action="store_true")
    ap.add_argument("--land-surface", choices=("bucket", "second_best"))
    a = ap.parse_args()

    def report(i, state):
        t = state["air_temperature"].values.ravel()
        rain = "  precipitation %8.3f mm/day" % state["convective_precipitation_rate"].values.ravel()[0] if a.moist_convection else ""
        if a.simple_physics:
            rain += "  stratiform %8.3f mm/day  LH %7.2f  SH %7.2f W m^-2" % (
                state["stratiform_precipitation_rate"].values.ravel()[0] * 8.64e7, state["surface_upward_latent_heat_flux"].values.ravel()[0],
                state["surface_upward_sensible_heat_flux"].values.ravel()[0])
        print("step %4d  T(surface) %8.3f K  T(surface layer) %8.3f K  T(top) %8.3f K  OLR %8.3f  SW heating(top) %7.3f K/day  LW heating(top) %8.3f K/day%s" % (
            i, state["surface_temperature"].values.ravel()[0], t[0], t[-1], state["upwelling_longwave_flux_in_air"].values.ravel()[-1],
            state["air_temperature_tendency_from_shortwave"].values.ravel()[-1],
            state["air_temperature_tendency_from_longwave"].values.ravel()[-1], rain))
    if a.grid_scale_condensation and a.simple_physics:
        ap.error("--grid-scale-condensation and --simple-physics are exclusive")
    run(a.steps, a.device_resident, report, a.boundary_layer, a.moist_convection, a.simple_physics, a.gray_longwave, a.grid_scale_condensation, a.sea_ice, a.land_surface, a.cork_longwave, a.cork_shortwave)


if __name__ == "__main__":
    main()
