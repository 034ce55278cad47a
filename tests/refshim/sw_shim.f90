! TEST INFRASTRUCTURE ONLY.  Our own bind(c) driver around the REFERENCE's shortwave module procedures, for what the
! reference computes and its binder does not return or accept: the direct / diffuse and UV-visible / near-IR sums, the
! fluxes of ONE band, and a surface albedo per band.  Per column and in driver order it calls inatm_sw -> cldprop_sw
! (cldprmc_sw on McICA sub-columns) -> setcoef_sw -> the iaer 0 / 10 aerosol copy -> spcvrt_sw (spcvmc_sw), as
! rrtmg_sw_rad.nomcica.f90:587-794 and rrtmg_sw_rad.f90:616-819 do, with two differences from the reference's driver:
!   * albdir / albdif come from the caller, albdir_in(ncol, nbndsw) / albdif_in(ncol, nbndsw) (C layout [14][ncol], band
!     index = the reference's band order); filled by the driver's band rule (rrtmg_sw_rad.nomcica.f90:648-659) from four
!     broadband numbers the outputs equal the binder's bit for bit;
!   * band = 0: spcvrt_sw (spcvmc_sw) runs once over the full band range (iout = 0), as the driver pins it; band = 1..14:
!     over that band alone (istart = iend = iout = jpb1-1+band: the g-point counter restarts at the band).
! Compiled against the reference's .mod files and linked against its shared library by tests/refshim/build.sh, so that the
! module state set through the reference binder (rrtmg_sw_set_constants, rrtmg_sw_ini_wrapper) is the state these
! procedures read.
!
! Arguments follow rrtmg_sw_{nomcica,mcica}_wrapper of the binder (iaer 6 is not supported here), the four albedos replaced
! by the two per-band arrays.  Outputs: rows(ncol, nlay+1, 14), level 1 = surface, the reference's accumulators in this
! order: zbbfu zbbfd zbbcu zbbcd zbbfddir zbbcddir zuvfd zuvcd zuvfddir zuvcddir znifd znicd znifddir znicddir; and
! hr(ncol, nlay, 2) = swhr, swhrc by the reference driver's formula (rrtmg_sw_rad.nomcica.f90:796-807) from rows 1-4.
module sw_shim
  use iso_c_binding
  use parkind, only : im => kind_im, rb => kind_rb
  use parrrsw, only : nbndsw, ngptsw, mxmol, jpband, jpb1, jpb2
  implicit none
  integer, parameter :: nrows = 14
  real(kind=rb), parameter :: zepzen = 1.e-10_rb
contains

  subroutine aerosol_copy(iaer, nlayers, taua, ssaa, asma, ztaua, zasya, zomga)
    integer(kind=im), intent(in) :: iaer, nlayers
    real(kind=rb), intent(in) :: taua(:,:), ssaa(:,:), asma(:,:)
    real(kind=rb), intent(out) :: ztaua(:,:), zasya(:,:), zomga(:,:)
    integer(kind=im) :: i, ib
    ztaua = 0._rb; zasya = 0._rb; zomga = 1._rb
    if (iaer .eq. 10) then
      do i = 1, nlayers
        do ib = 1, nbndsw
          ztaua(i,ib) = taua(i,ib)
          zasya(i,ib) = asma(i,ib)
          zomga(i,ib) = ssaa(i,ib)
        enddo
      enddo
    endif
  end subroutine aerosol_copy

  subroutine band_range(band, istart, iend, iout)
    integer(kind=im), intent(in) :: band
    integer(kind=im), intent(out) :: istart, iend, iout
    if (band .eq. 0) then
      istart = jpb1; iend = jpb2; iout = 0
    else
      istart = jpb1-1+band; iend = istart; iout = istart
    endif
  end subroutine band_range

  subroutine store_column(iplon, nlayers, z, pdp, rows, hr)
    use rrsw_con, only : heatfac
    integer(kind=im), intent(in) :: iplon, nlayers
    real(kind=rb), intent(in) :: z(:,:), pdp(:)
    real(kind=rb), intent(inout) :: rows(:,:,:), hr(:,:,:)
    real(kind=rb) :: swnflx(nlayers+1), swnflxc(nlayers+1), zdpgcp
    integer(kind=im) :: i
    rows(iplon,:,:) = z(1:nlayers+1,:)
    do i = 1, nlayers+1
      swnflxc(i) = z(i,4) - z(i,3)
      swnflx(i) = z(i,2) - z(i,1)
    enddo
    do i = 1, nlayers
      zdpgcp = heatfac / pdp(i)
      hr(iplon,i,2) = (swnflxc(i+1) - swnflxc(i)) * zdpgcp
      hr(iplon,i,1) = (swnflx(i+1) - swnflx(i)) * zdpgcp
    enddo
  end subroutine store_column

  subroutine sw_shim_nomcica(ncol, nlay, icld_in, iaer_in, play, plev, tlay, tlev, tsfc, &
      h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, albdir_in, albdif_in, coszen, adjes, dyofyr, scon, isolvar, &
      inflgsw, iceflgsw, liqflgsw, cldfr, taucld, ssacld, asmcld, fsfcld, cicewp, cliqwp, reice, reliq, &
      tauaer, ssaaer, asmaer, bndsolvar, indsolvar, solcycfrac, band, rows, hr) bind(c)
    use rrtmg_sw_rad_nomcica, only : inatm_sw
    use rrtmg_sw_cldprop, only : cldprop_sw
    use rrtmg_sw_setcoef, only : setcoef_sw
    use rrtmg_sw_spcvrt, only : spcvrt_sw
    integer(kind=im), intent(in) :: ncol, nlay, icld_in, iaer_in, dyofyr, isolvar, inflgsw, iceflgsw, liqflgsw, band
    real(kind=rb), intent(in) :: play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol)
    real(kind=rb), intent(in) :: h2ovmr(ncol,nlay), o3vmr(ncol,nlay), co2vmr(ncol,nlay), ch4vmr(ncol,nlay), n2ovmr(ncol,nlay), o2vmr(ncol,nlay)
    real(kind=rb), intent(in) :: albdir_in(ncol,nbndsw), albdif_in(ncol,nbndsw), coszen(ncol), adjes, scon, solcycfrac
    real(kind=rb), intent(in) :: cldfr(ncol,nlay)
    real(kind=rb), intent(in) :: taucld(nbndsw,ncol,nlay), ssacld(nbndsw,ncol,nlay), asmcld(nbndsw,ncol,nlay), fsfcld(nbndsw,ncol,nlay)
    real(kind=rb), intent(in) :: cicewp(ncol,nlay), cliqwp(ncol,nlay), reice(ncol,nlay), reliq(ncol,nlay)
    real(kind=rb), intent(in) :: tauaer(ncol,nlay,nbndsw), ssaaer(ncol,nlay,nbndsw), asmaer(ncol,nlay,nbndsw)
    real(kind=rb), intent(in) :: bndsolvar(nbndsw)
    real(kind=rb), intent(inout) :: indsolvar(2)
    real(kind=rb), intent(out) :: rows(ncol,nlay+1,nrows), hr(ncol,nlay,2)
    integer(kind=im) :: istart, iend, iout
    integer(kind=im) :: icld, iaer, iplon, i, ib, nlayers, inflag, iceflag, liqflag, laytrop, layswtch, laylow
    integer(kind=im) :: jp(nlay+1), jt(nlay+1), jt1(nlay+1), indself(nlay+1), indfor(nlay+1)
    real(kind=rb) :: pavel(nlay+1), tavel(nlay+1), pz(0:nlay+1), tz(0:nlay+1), tbound, pdp(nlay+1), coldry(nlay+1)
    real(kind=rb) :: wkl(mxmol,nlay+1), cossza, adjflux(jpband), albdir(nbndsw), albdif(nbndsw)
    real(kind=rb) :: taua(nlay+1,nbndsw), ssaa(nlay+1,nbndsw), asma(nlay+1,nbndsw)
    real(kind=rb), dimension(nlay+1) :: colh2o, colco2, colo3, coln2o, colch4, colo2, colmol, co2mult, &
         selffac, selffrac, forfac, forfrac, fac00, fac01, fac10, fac11
    real(kind=rb) :: cldfrac(nlay+1), tauc(nbndsw,nlay+1), ssac(nbndsw,nlay+1), asmc(nbndsw,nlay+1), fsfc(nbndsw,nlay+1)
    real(kind=rb) :: ciwp(nlay+1), clwp(nlay+1), rel(nlay+1), rei(nlay+1)
    real(kind=rb) :: taucloud(nlay+1,jpband), taucldorig(nlay+1,jpband), ssacloud(nlay+1,jpband), asmcloud(nlay+1,jpband)
    real(kind=rb), dimension(nlay+1,nbndsw) :: ztauc, ztaucorig, zasyc, zomgc, ztaua, zasya, zomga
    real(kind=rb) :: z(nlay+2,nrows)
    real(kind=rb) :: svar_f, svar_s, svar_i, svar_f_bnd(jpband), svar_s_bnd(jpband), svar_i_bnd(jpband)
    icld = icld_in; iaer = iaer_in
    if (icld.lt.0.or.icld.gt.3) icld = 2
    if (iaer.ne.0.and.iaer.ne.6.and.iaer.ne.10) iaer = 0
    call band_range(band, istart, iend, iout)
    do iplon = 1, ncol
      call inatm_sw(iplon, nlay, icld, iaer, play, plev, tlay, tlev, tsfc, h2ovmr, &
           o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, adjes, dyofyr, scon, isolvar, inflgsw, iceflgsw, liqflgsw, &
           cldfr, taucld, ssacld, asmcld, fsfcld, cicewp, cliqwp, reice, reliq, tauaer, ssaaer, asmaer, &
           nlayers, pavel, pz, pdp, tavel, tz, tbound, coldry, wkl, adjflux, inflag, iceflag, liqflag, cldfrac, tauc, &
           ssac, asmc, fsfc, ciwp, clwp, rei, rel, taua, ssaa, asma, &
           svar_f, svar_s, svar_i, svar_f_bnd, svar_s_bnd, svar_i_bnd, bndsolvar, indsolvar, solcycfrac)
      ! (the driver stops on partial cloud here: the inputs of this shim are clear or overcast)
      call cldprop_sw(nlayers, inflag, iceflag, liqflag, cldfrac, tauc, ssac, asmc, fsfc, ciwp, clwp, rei, rel, &
                      taucldorig, taucloud, ssacloud, asmcloud)
      call setcoef_sw(nlayers, pavel, tavel, pz, tz, tbound, coldry, wkl, laytrop, layswtch, laylow, jp, jt, jt1, &
                      co2mult, colch4, colco2, colh2o, colmol, coln2o, colo2, colo3, fac00, fac01, fac10, fac11, &
                      selffac, selffrac, indself, forfac, forfrac, indfor)
      cossza = coszen(iplon)
      if (cossza .lt. zepzen) cossza = zepzen
      albdir(:) = albdir_in(iplon,:); albdif(:) = albdif_in(iplon,:)
      if (icld.eq.0) then
        ztauc = 0._rb; ztaucorig = 0._rb; zasyc = 0._rb; zomgc = 1._rb
      else
        do i = 1, nlayers
          do ib = 1, nbndsw
            ztauc(i,ib) = taucloud(i,jpb1-1+ib)
            ztaucorig(i,ib) = taucldorig(i,jpb1-1+ib)
            zasyc(i,ib) = asmcloud(i,jpb1-1+ib)
            zomgc(i,ib) = ssacloud(i,jpb1-1+ib)
          enddo
        enddo
      endif
      call aerosol_copy(iaer, nlayers, taua, ssaa, asma, ztaua, zasya, zomga)
      z = 0._rb
      call spcvrt_sw(nlayers, istart, iend, 1, 1, iout, pavel, tavel, pz, tz, tbound, albdif, albdir, &
           cldfrac, ztauc, zasyc, zomgc, ztaucorig, ztaua, zasya, zomga, cossza, coldry, wkl, adjflux, &
           isolvar, svar_f, svar_s, svar_i, svar_f_bnd, svar_s_bnd, svar_i_bnd, &
           laytrop, layswtch, laylow, jp, jt, jt1, co2mult, colch4, colco2, colh2o, colmol, coln2o, colo2, colo3, &
           fac00, fac01, fac10, fac11, selffac, selffrac, indself, forfac, forfrac, indfor, &
           z(:,2), z(:,1), z(:,4), z(:,3), z(:,7), z(:,8), z(:,11), z(:,12), &
           z(:,5), z(:,6), z(:,9), z(:,10), z(:,13), z(:,14))
      call store_column(iplon, nlayers, z, pdp, rows, hr)
    enddo
  end subroutine sw_shim_nomcica

  subroutine sw_shim_mcica(ncol, nlay, icld_in, iaer_in, play, plev, tlay, tlev, tsfc, &
      h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, albdir_in, albdif_in, coszen, adjes, dyofyr, scon, isolvar, &
      inflgsw, iceflgsw, liqflgsw, cldfmcl, taucmcl, ssacmcl, asmcmcl, fsfcmcl, ciwpmcl, clwpmcl, reicmcl, relqmcl, &
      tauaer, ssaaer, asmaer, bndsolvar, indsolvar, solcycfrac, band, rows, hr) bind(c)
    use rrtmg_sw_rad, only : inatm_sw
    use rrtmg_sw_cldprmc, only : cldprmc_sw
    use rrtmg_sw_setcoef, only : setcoef_sw
    use rrtmg_sw_spcvmc, only : spcvmc_sw
    integer(kind=im), intent(in) :: ncol, nlay, icld_in, iaer_in, dyofyr, isolvar, inflgsw, iceflgsw, liqflgsw, band
    real(kind=rb), intent(in) :: play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol)
    real(kind=rb), intent(in) :: h2ovmr(ncol,nlay), o3vmr(ncol,nlay), co2vmr(ncol,nlay), ch4vmr(ncol,nlay), n2ovmr(ncol,nlay), o2vmr(ncol,nlay)
    real(kind=rb), intent(in) :: albdir_in(ncol,nbndsw), albdif_in(ncol,nbndsw), coszen(ncol), adjes, scon, solcycfrac
    real(kind=rb), intent(in) :: cldfmcl(ngptsw,ncol,nlay), taucmcl(ngptsw,ncol,nlay), ssacmcl(ngptsw,ncol,nlay)
    real(kind=rb), intent(in) :: asmcmcl(ngptsw,ncol,nlay), fsfcmcl(ngptsw,ncol,nlay), ciwpmcl(ngptsw,ncol,nlay), clwpmcl(ngptsw,ncol,nlay)
    real(kind=rb), intent(in) :: reicmcl(ncol,nlay), relqmcl(ncol,nlay)
    real(kind=rb), intent(in) :: tauaer(ncol,nlay,nbndsw), ssaaer(ncol,nlay,nbndsw), asmaer(ncol,nlay,nbndsw)
    real(kind=rb), intent(in) :: bndsolvar(nbndsw)
    real(kind=rb), intent(inout) :: indsolvar(2)
    real(kind=rb), intent(out) :: rows(ncol,nlay+1,nrows), hr(ncol,nlay,2)
    integer(kind=im) :: istart, iend, iout
    integer(kind=im) :: icld, iaer, iplon, i, ig, nlayers, inflag, iceflag, liqflag, laytrop, layswtch, laylow
    integer(kind=im) :: jp(nlay+1), jt(nlay+1), jt1(nlay+1), indself(nlay+1), indfor(nlay+1)
    real(kind=rb) :: pavel(nlay+1), tavel(nlay+1), pz(0:nlay+1), tz(0:nlay+1), tbound, pdp(nlay+1), coldry(nlay+1)
    real(kind=rb) :: wkl(mxmol,nlay+1), cossza, adjflux(jpband), albdir(nbndsw), albdif(nbndsw)
    real(kind=rb) :: taua(nlay+1,nbndsw), ssaa(nlay+1,nbndsw), asma(nlay+1,nbndsw)
    real(kind=rb), dimension(nlay+1) :: colh2o, colco2, colo3, coln2o, colch4, colo2, colmol, co2mult, &
         selffac, selffrac, forfac, forfrac, fac00, fac01, fac10, fac11
    real(kind=rb), dimension(ngptsw,nlay+1) :: cldfmc, ciwpmc, clwpmc, taucmc, taormc, ssacmc, asmcmc, fsfcmc
    real(kind=rb) :: relqmc(nlay+1), reicmc(nlay+1)
    real(kind=rb), dimension(nlay+1,ngptsw) :: zcldfmc, ztaucmc, ztaormc, zasycmc, zomgcmc
    real(kind=rb), dimension(nlay+1,nbndsw) :: ztaua, zasya, zomga
    real(kind=rb) :: z(nlay+2,nrows)
    real(kind=rb) :: svar_f, svar_s, svar_i, svar_f_bnd(jpband), svar_s_bnd(jpband), svar_i_bnd(jpband)
    icld = icld_in; iaer = iaer_in
    if (icld.lt.0.or.icld.gt.3) icld = 2
    if (iaer.ne.0.and.iaer.ne.6.and.iaer.ne.10) iaer = 0
    call band_range(band, istart, iend, iout)
    do iplon = 1, ncol
      call inatm_sw(iplon, nlay, icld, iaer, play, plev, tlay, tlev, tsfc, h2ovmr, &
           o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, adjes, dyofyr, scon, isolvar, inflgsw, iceflgsw, liqflgsw, &
           cldfmcl, taucmcl, ssacmcl, asmcmcl, fsfcmcl, ciwpmcl, clwpmcl, reicmcl, relqmcl, tauaer, ssaaer, asmaer, &
           nlayers, pavel, pz, pdp, tavel, tz, tbound, coldry, wkl, adjflux, inflag, iceflag, liqflag, cldfmc, taucmc, &
           ssacmc, asmcmc, fsfcmc, ciwpmc, clwpmc, reicmc, relqmc, taua, ssaa, asma, &
           svar_f, svar_s, svar_i, svar_f_bnd, svar_s_bnd, svar_i_bnd, bndsolvar, indsolvar, solcycfrac)
      call cldprmc_sw(nlayers, inflag, iceflag, liqflag, cldfmc, ciwpmc, clwpmc, reicmc, relqmc, &
                      taormc, taucmc, ssacmc, asmcmc, fsfcmc)
      call setcoef_sw(nlayers, pavel, tavel, pz, tz, tbound, coldry, wkl, laytrop, layswtch, laylow, jp, jt, jt1, &
                      co2mult, colch4, colco2, colh2o, colmol, coln2o, colo2, colo3, fac00, fac01, fac10, fac11, &
                      selffac, selffrac, indself, forfac, forfrac, indfor)
      cossza = coszen(iplon)
      if (cossza .lt. zepzen) cossza = zepzen
      albdir(:) = albdir_in(iplon,:); albdif(:) = albdif_in(iplon,:)
      if (icld.eq.0) then
        zcldfmc = 0._rb; ztaucmc = 0._rb; ztaormc = 0._rb; zasycmc = 0._rb; zomgcmc = 1._rb
      else
        do i = 1, nlayers
          do ig = 1, ngptsw
            zcldfmc(i,ig) = cldfmc(ig,i)
            ztaucmc(i,ig) = taucmc(ig,i)
            ztaormc(i,ig) = taormc(ig,i)
            zasycmc(i,ig) = asmcmc(ig,i)
            zomgcmc(i,ig) = ssacmc(ig,i)
          enddo
        enddo
      endif
      call aerosol_copy(iaer, nlayers, taua, ssaa, asma, ztaua, zasya, zomga)
      z = 0._rb
      call spcvmc_sw(nlayers, istart, iend, 1, 1, iout, pavel, tavel, pz, tz, tbound, albdif, albdir, &
           zcldfmc, ztaucmc, zasycmc, zomgcmc, ztaormc, ztaua, zasya, zomga, cossza, coldry, wkl, adjflux, &
           isolvar, svar_f, svar_s, svar_i, svar_f_bnd, svar_s_bnd, svar_i_bnd, &
           laytrop, layswtch, laylow, jp, jt, jt1, co2mult, colch4, colco2, colh2o, colmol, coln2o, colo2, colo3, &
           fac00, fac01, fac10, fac11, selffac, selffrac, indself, forfac, forfrac, indfor, &
           z(:,2), z(:,1), z(:,4), z(:,3), z(:,7), z(:,8), z(:,11), z(:,12), &
           z(:,5), z(:,6), z(:,9), z(:,10), z(:,13), z(:,14))
      call store_column(iplon, nlayers, z, pdp, rows, hr)
    enddo
  end subroutine sw_shim_mcica
end module sw_shim
