! TEST INFRASTRUCTURE ONLY.  Our own bind(c) driver around the REFERENCE's longwave module procedures, for the fluxes BY
! BAND: the reference's rtrn / rtrnmr / rtrnmc take a band range (istart, iend) and restart their g-point counter at the band
! when iout > 0, but its driver pins them to all bands.  Per column and in driver order it calls inatm -> cldprop (cldprmc
! on McICA sub-columns) -> setcoef (istart = 1, as the driver) -> taumol -> the aerosol sum, as rrtmg_lw_rad.nomcica.f90:
! 458-541 and rrtmg_lw_rad.f90:472-548 do, and then the transfer routine once over the full range (iout = 0: slot 0, checked
! against the binder's outputs bit for bit) and once per band with istart = iend = iout = band (slots 1..16).  Compiled
! against the reference's .mod files and linked against its shared library by tests/refshim/build.sh, so that the
! module state set through the reference binder (rrtmg_set_constants, the k-tables, rrtmg_lw_ini_wrapper) is the state these
! procedures read.
!
! Arguments follow rrtmg_lw_{nomcica,mcica}_wrapper of the binder.  Output: bands(ncol, nlay+1, 4, 0:16), level 1 =
! surface, the four fluxes in this order: totuflux totdflux totuclfl totdclfl.
module lw_bands_shim
  use iso_c_binding
  use parkind, only : im => kind_im, rb => kind_rb
  use parrrtm, only : nbndlw, ngptlw, mxmol, maxxsec
  implicit none
  integer, parameter :: nout = 4
contains

  subroutine lw_bands_nomcica(ncol, nlay, icld_in, idrv, play, plev, tlay, tlev, tsfc, &
      h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, &
      inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, tauaer, bands) bind(c)
    use rrlw_con, only : fluxfac, oneminus, pi
    use rrlw_wvn, only : ngb
    use rrtmg_lw_rad_nomcica, only : inatm
    use rrtmg_lw_cldprop, only : cldprop
    use rrtmg_lw_setcoef, only : setcoef
    use rrtmg_lw_taumol, only : taumol
    use rrtmg_lw_rtrn, only : rtrn
    use rrtmg_lw_rtrnmr, only : rtrnmr
    integer(kind=im), intent(in) :: ncol, nlay, icld_in, idrv, inflglw, iceflglw, liqflglw
    real(kind=rb), intent(in) :: play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol)
    real(kind=rb), intent(in) :: h2ovmr(ncol,nlay), o3vmr(ncol,nlay), co2vmr(ncol,nlay), ch4vmr(ncol,nlay), n2ovmr(ncol,nlay), o2vmr(ncol,nlay)
    real(kind=rb), intent(in) :: cfc11vmr(ncol,nlay), cfc12vmr(ncol,nlay), cfc22vmr(ncol,nlay), ccl4vmr(ncol,nlay), emis(ncol,nbndlw)
    real(kind=rb), intent(in) :: cldfr(ncol,nlay), taucld(nbndlw,ncol,nlay), cicewp(ncol,nlay), cliqwp(ncol,nlay), reice(ncol,nlay), reliq(ncol,nlay)
    real(kind=rb), intent(in) :: tauaer(ncol,nlay,nbndlw)
    real(kind=rb), intent(out) :: bands(ncol,nlay+1,nout,0:nbndlw)
    integer(kind=im) :: icld, iaer, iplon, k, ig, kb, i1, i2, io, istart
    integer(kind=im) :: nlayers, inflag, iceflag, liqflag, laytrop, ncbands
    real(kind=rb) :: pavel(nlay+1), tavel(nlay+1), pz(0:nlay+1), tz(0:nlay+1), tbound, coldry(nlay+1), wbrodl(nlay+1)
    real(kind=rb) :: wkl(mxmol,nlay+1), wx(maxxsec,nlay+1), pwvcm, semiss(nbndlw), taua(nlay+1,nbndlw)
    real(kind=rb) :: cldfrac(nlay+1), tauc(nbndlw,nlay+1), ciwp(nlay+1), clwp(nlay+1), rei(nlay+1), rel(nlay+1), taucloud(nlay+1,nbndlw)
    integer(kind=im) :: jp(nlay+1), jt(nlay+1), jt1(nlay+1), indself(nlay+1), indfor(nlay+1), indminor(nlay+1)
    real(kind=rb) :: planklay(nlay+1,nbndlw), planklev(0:nlay+1,nbndlw), plankbnd(nbndlw), dplankbnd_dt(nbndlw)
    real(kind=rb), dimension(nlay+1) :: colh2o, colco2, colo3, coln2o, colco, colch4, colo2, colbrd, fac00, fac01, fac10, fac11, &
         rat_h2oco2, rat_h2oco2_1, rat_h2oo3, rat_h2oo3_1, rat_h2on2o, rat_h2on2o_1, rat_h2och4, rat_h2och4_1, &
         rat_n2oco2, rat_n2oco2_1, rat_o3co2, rat_o3co2_1, selffac, selffrac, forfac, forfrac, minorfrac, scaleminor, scaleminorn2
    real(kind=rb) :: fracs(nlay+1,ngptlw), taug(nlay+1,ngptlw), taut(nlay+1,ngptlw)
    real(kind=rb), dimension(0:nlay+1) :: totuflux, totdflux, fnet, htr, totuclfl, totdclfl, fnetc, htrc, dtotuflux_dt, dtotuclfl_dt
    oneminus = 1._rb - 1.e-6_rb
    pi = 2._rb*asin(1._rb)
    fluxfac = pi * 2.e4_rb
    istart = 1
    icld = icld_in
    if (icld.lt.0.or.icld.gt.3) icld = 2
    iaer = 10
    do iplon = 1, ncol
      call inatm (iplon, nlay, icld, iaer, play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, &
                  cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, iceflglw, liqflglw, &
                  cldfr, taucld, cicewp, cliqwp, reice, reliq, tauaer, &
                  nlayers, pavel, pz, tavel, tz, tbound, semiss, coldry, wkl, wbrodl, wx, pwvcm, inflag, iceflag, liqflag, &
                  cldfrac, tauc, ciwp, clwp, rei, rel, taua)
      call cldprop(nlayers, inflag, iceflag, liqflag, cldfrac, tauc, ciwp, clwp, rei, rel, ncbands, taucloud)
      call setcoef(nlayers, istart, pavel, tavel, tz, tbound, semiss, coldry, wkl, wbrodl, &
                   laytrop, jp, jt, jt1, planklay, planklev, plankbnd, idrv, dplankbnd_dt, &
                   colh2o, colco2, colo3, coln2o, colco, colch4, colo2, colbrd, fac00, fac01, fac10, fac11, &
                   rat_h2oco2, rat_h2oco2_1, rat_h2oo3, rat_h2oo3_1, rat_h2on2o, rat_h2on2o_1, rat_h2och4, rat_h2och4_1, &
                   rat_n2oco2, rat_n2oco2_1, rat_o3co2, rat_o3co2_1, selffac, selffrac, indself, forfac, forfrac, indfor, &
                   minorfrac, scaleminor, scaleminorn2, indminor)
      call taumol(nlayers, pavel, wx, coldry, laytrop, jp, jt, jt1, planklay, planklev, plankbnd, &
                  colh2o, colco2, colo3, coln2o, colco, colch4, colo2, colbrd, fac00, fac01, fac10, fac11, &
                  rat_h2oco2, rat_h2oco2_1, rat_h2oo3, rat_h2oo3_1, rat_h2on2o, rat_h2on2o_1, rat_h2och4, rat_h2och4_1, &
                  rat_n2oco2, rat_n2oco2_1, rat_o3co2, rat_o3co2_1, selffac, selffrac, indself, forfac, forfrac, indfor, &
                  minorfrac, scaleminor, scaleminorn2, indminor, fracs, taug)
      do k = 1, nlayers
        do ig = 1, ngptlw
          taut(k,ig) = taug(k,ig) + taua(k,ngb(ig))
        enddo
      enddo
      do kb = 0, nbndlw
        if (kb .eq. 0) then
          i1 = 1; i2 = nbndlw; io = 0
        else
          i1 = kb; i2 = kb; io = kb
        endif
        if (icld .eq. 1) then
          call rtrn(nlayers, i1, i2, io, pz, semiss, ncbands, cldfrac, taucloud, planklay, planklev, plankbnd, &
                    pwvcm, fracs, taut, totuflux, totdflux, fnet, htr, totuclfl, totdclfl, fnetc, htrc, &
                    idrv, dplankbnd_dt, dtotuflux_dt, dtotuclfl_dt)
        else
          call rtrnmr(nlayers, i1, i2, io, pz, semiss, ncbands, cldfrac, taucloud, planklay, planklev, plankbnd, &
                      pwvcm, fracs, taut, totuflux, totdflux, fnet, htr, totuclfl, totdclfl, fnetc, htrc, &
                      idrv, dplankbnd_dt, dtotuflux_dt, dtotuclfl_dt)
        endif
        do k = 0, nlayers
          bands(iplon,k+1,1,kb) = totuflux(k)
          bands(iplon,k+1,2,kb) = totdflux(k)
          bands(iplon,k+1,3,kb) = totuclfl(k)
          bands(iplon,k+1,4,kb) = totdclfl(k)
        enddo
      enddo
    enddo
  end subroutine lw_bands_nomcica

  subroutine lw_bands_mcica(ncol, nlay, icld_in, idrv, play, plev, tlay, tlev, tsfc, &
      h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, &
      inflglw, iceflglw, liqflglw, cldfmcl, taucmcl, ciwpmcl, clwpmcl, reicmcl, relqmcl, tauaer, bands) bind(c)
    use rrlw_con, only : fluxfac, oneminus, pi
    use rrlw_wvn, only : ngb
    use rrtmg_lw_rad, only : inatm
    use rrtmg_lw_cldprmc, only : cldprmc
    use rrtmg_lw_setcoef, only : setcoef
    use rrtmg_lw_taumol, only : taumol
    use rrtmg_lw_rtrnmc, only : rtrnmc
    integer(kind=im), intent(in) :: ncol, nlay, icld_in, idrv, inflglw, iceflglw, liqflglw
    real(kind=rb), intent(in) :: play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol)
    real(kind=rb), intent(in) :: h2ovmr(ncol,nlay), o3vmr(ncol,nlay), co2vmr(ncol,nlay), ch4vmr(ncol,nlay), n2ovmr(ncol,nlay), o2vmr(ncol,nlay)
    real(kind=rb), intent(in) :: cfc11vmr(ncol,nlay), cfc12vmr(ncol,nlay), cfc22vmr(ncol,nlay), ccl4vmr(ncol,nlay), emis(ncol,nbndlw)
    real(kind=rb), intent(in) :: cldfmcl(ngptlw,ncol,nlay), taucmcl(ngptlw,ncol,nlay), ciwpmcl(ngptlw,ncol,nlay), clwpmcl(ngptlw,ncol,nlay)
    real(kind=rb), intent(in) :: reicmcl(ncol,nlay), relqmcl(ncol,nlay)
    real(kind=rb), intent(in) :: tauaer(ncol,nlay,nbndlw)
    real(kind=rb), intent(out) :: bands(ncol,nlay+1,nout,0:nbndlw)
    integer(kind=im) :: icld, iaer, iplon, k, ig, kb, i1, i2, io, istart
    integer(kind=im) :: nlayers, inflag, iceflag, liqflag, laytrop, ncbands
    real(kind=rb) :: pavel(nlay+1), tavel(nlay+1), pz(0:nlay+1), tz(0:nlay+1), tbound, coldry(nlay+1), wbrodl(nlay+1)
    real(kind=rb) :: wkl(mxmol,nlay+1), wx(maxxsec,nlay+1), pwvcm, semiss(nbndlw), taua(nlay+1,nbndlw)
    real(kind=rb), dimension(ngptlw,nlay+1) :: cldfmc, ciwpmc, clwpmc, taucmc
    real(kind=rb) :: relqmc(nlay+1), reicmc(nlay+1)
    integer(kind=im) :: jp(nlay+1), jt(nlay+1), jt1(nlay+1), indself(nlay+1), indfor(nlay+1), indminor(nlay+1)
    real(kind=rb) :: planklay(nlay+1,nbndlw), planklev(0:nlay+1,nbndlw), plankbnd(nbndlw), dplankbnd_dt(nbndlw)
    real(kind=rb), dimension(nlay+1) :: colh2o, colco2, colo3, coln2o, colco, colch4, colo2, colbrd, fac00, fac01, fac10, fac11, &
         rat_h2oco2, rat_h2oco2_1, rat_h2oo3, rat_h2oo3_1, rat_h2on2o, rat_h2on2o_1, rat_h2och4, rat_h2och4_1, &
         rat_n2oco2, rat_n2oco2_1, rat_o3co2, rat_o3co2_1, selffac, selffrac, forfac, forfrac, minorfrac, scaleminor, scaleminorn2
    real(kind=rb) :: fracs(nlay+1,ngptlw), taug(nlay+1,ngptlw), taut(nlay+1,ngptlw)
    real(kind=rb), dimension(0:nlay+1) :: totuflux, totdflux, fnet, htr, totuclfl, totdclfl, fnetc, htrc, dtotuflux_dt, dtotuclfl_dt
    oneminus = 1._rb - 1.e-6_rb
    pi = 2._rb * asin(1._rb)
    fluxfac = pi * 2.e4_rb
    istart = 1
    icld = icld_in
    if (icld.lt.0.or.icld.gt.3) icld = 2
    iaer = 10
    do iplon = 1, ncol
      call inatm (iplon, nlay, icld, iaer, play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, &
                  cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, iceflglw, liqflglw, &
                  cldfmcl, taucmcl, ciwpmcl, clwpmcl, reicmcl, relqmcl, tauaer, &
                  nlayers, pavel, pz, tavel, tz, tbound, semiss, coldry, wkl, wbrodl, wx, pwvcm, inflag, iceflag, liqflag, &
                  cldfmc, taucmc, ciwpmc, clwpmc, reicmc, relqmc, taua)
      call cldprmc(nlayers, inflag, iceflag, liqflag, cldfmc, ciwpmc, clwpmc, reicmc, relqmc, ncbands, taucmc)
      call setcoef(nlayers, istart, pavel, tavel, tz, tbound, semiss, coldry, wkl, wbrodl, &
                   laytrop, jp, jt, jt1, planklay, planklev, plankbnd, idrv, dplankbnd_dt, &
                   colh2o, colco2, colo3, coln2o, colco, colch4, colo2, colbrd, fac00, fac01, fac10, fac11, &
                   rat_h2oco2, rat_h2oco2_1, rat_h2oo3, rat_h2oo3_1, rat_h2on2o, rat_h2on2o_1, rat_h2och4, rat_h2och4_1, &
                   rat_n2oco2, rat_n2oco2_1, rat_o3co2, rat_o3co2_1, selffac, selffrac, indself, forfac, forfrac, indfor, &
                   minorfrac, scaleminor, scaleminorn2, indminor)
      call taumol(nlayers, pavel, wx, coldry, laytrop, jp, jt, jt1, planklay, planklev, plankbnd, &
                  colh2o, colco2, colo3, coln2o, colco, colch4, colo2, colbrd, fac00, fac01, fac10, fac11, &
                  rat_h2oco2, rat_h2oco2_1, rat_h2oo3, rat_h2oo3_1, rat_h2on2o, rat_h2on2o_1, rat_h2och4, rat_h2och4_1, &
                  rat_n2oco2, rat_n2oco2_1, rat_o3co2, rat_o3co2_1, selffac, selffrac, indself, forfac, forfrac, indfor, &
                  minorfrac, scaleminor, scaleminorn2, indminor, fracs, taug)
      do k = 1, nlayers
        do ig = 1, ngptlw
          taut(k,ig) = taug(k,ig) + taua(k,ngb(ig))
        enddo
      enddo
      do kb = 0, nbndlw
        if (kb .eq. 0) then
          i1 = 1; i2 = nbndlw; io = 0
        else
          i1 = kb; i2 = kb; io = kb
        endif
        call rtrnmc(nlayers, i1, i2, io, pz, semiss, ncbands, cldfmc, taucmc, planklay, planklev, plankbnd, &
                    pwvcm, fracs, taut, totuflux, totdflux, fnet, htr, totuclfl, totdclfl, fnetc, htrc, &
                    idrv, dplankbnd_dt, dtotuflux_dt, dtotuclfl_dt)
        do k = 0, nlayers
          bands(iplon,k+1,1,kb) = totuflux(k)
          bands(iplon,k+1,2,kb) = totdflux(k)
          bands(iplon,k+1,3,kb) = totuclfl(k)
          bands(iplon,k+1,4,kb) = totdclfl(k)
        enddo
      enddo
    enddo
  end subroutine lw_bands_mcica
end module lw_bands_shim
