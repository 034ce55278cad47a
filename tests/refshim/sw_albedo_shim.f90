! TEST INFRASTRUCTURE ONLY.  Our own bind(c) driver around the REFERENCE's shortwave module procedures, for the SURFACE
! ALBEDO BY BAND: the reference's spcvrt_sw / spcvmc_sw take albdir(nbndsw) / albdif(nbndsw), one value per band, but its
! driver fills them from four broadband numbers by a fixed rule (rrtmg_sw_rad.nomcica.f90:648-659).  This driver is
! sw_albedo_shim.f90's (inatm_sw -> cldprop_sw | cldprmc_sw -> setcoef_sw -> the iaer 0 / 10 aerosol copy, per column and in
! driver order) with ONE difference: albdir / albdif come from the caller, albdir_in(ncol, nbndsw) / albdif_in(ncol, nbndsw)
! (C layout [14][ncol], band index = the reference's band order).  spcvrt_sw (spcvmc_sw) runs once over the full band range
! (iout = 0); the six broadband outputs are returned, the heating rates by the reference driver's formula
! (rrtmg_sw_rad.nomcica.f90:796-807).  With albdir_in / albdif_in filled by the band rule the outputs equal the binder's bit
! for bit (tests/test_spectral_albedo.py).  Compiled against the reference's .mod files and linked against its shared
! library by tests/refshim/build_albedo.sh.
!
! Arguments follow rrtmg_sw_{nomcica,mcica}_wrapper of the binder (iaer 6 is not supported here), the four albedos replaced
! by the two per-band arrays.  Outputs: swuflx, swdflx, swuflxc, swdflxc (ncol, nlay+1), level 1 = surface; swhr, swhrc (ncol, nlay).
module sw_albedo_shim
  use iso_c_binding
  use parkind, only : im => kind_im, rb => kind_rb
  use parrrsw, only : nbndsw, ngptsw, mxmol, jpband, jpb1, jpb2
  implicit none
  integer, parameter :: ncomp = 14
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

  subroutine sw_albedo_nomcica(ncol, nlay, icld_in, iaer_in, play, plev, tlay, tlev, tsfc, &
      h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, albdir_in, albdif_in, coszen, adjes, dyofyr, scon, isolvar, &
      inflgsw, iceflgsw, liqflgsw, cldfr, taucld, ssacld, asmcld, fsfcld, cicewp, cliqwp, reice, reliq, &
      tauaer, ssaaer, asmaer, bndsolvar, indsolvar, solcycfrac, &
      swuflx, swdflx, swhr, swuflxc, swdflxc, swhrc) bind(c)
    use rrtmg_sw_rad_nomcica, only : inatm_sw
    use rrtmg_sw_cldprop, only : cldprop_sw
    use rrtmg_sw_setcoef, only : setcoef_sw
    use rrtmg_sw_spcvrt, only : spcvrt_sw
    use rrsw_con, only : heatfac
    integer(kind=im), intent(in) :: ncol, nlay, icld_in, iaer_in, dyofyr, isolvar, inflgsw, iceflgsw, liqflgsw
    real(kind=rb), intent(in) :: play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol)
    real(kind=rb), intent(in) :: h2ovmr(ncol,nlay), o3vmr(ncol,nlay), co2vmr(ncol,nlay), ch4vmr(ncol,nlay), n2ovmr(ncol,nlay), o2vmr(ncol,nlay)
    real(kind=rb), intent(in) :: albdir_in(ncol,nbndsw), albdif_in(ncol,nbndsw), coszen(ncol), adjes, scon, solcycfrac
    real(kind=rb), intent(in) :: cldfr(ncol,nlay)
    real(kind=rb), intent(in) :: taucld(nbndsw,ncol,nlay), ssacld(nbndsw,ncol,nlay), asmcld(nbndsw,ncol,nlay), fsfcld(nbndsw,ncol,nlay)
    real(kind=rb), intent(in) :: cicewp(ncol,nlay), cliqwp(ncol,nlay), reice(ncol,nlay), reliq(ncol,nlay)
    real(kind=rb), intent(in) :: tauaer(ncol,nlay,nbndsw), ssaaer(ncol,nlay,nbndsw), asmaer(ncol,nlay,nbndsw)
    real(kind=rb), intent(in) :: bndsolvar(nbndsw)
    real(kind=rb), intent(inout) :: indsolvar(2)
    real(kind=rb), intent(out) :: swuflx(ncol,nlay+1), swdflx(ncol,nlay+1), swhr(ncol,nlay), swuflxc(ncol,nlay+1), swdflxc(ncol,nlay+1), swhrc(ncol,nlay)
    real(kind=rb) :: swnflx(nlay+2), swnflxc(nlay+2), zdpgcp
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
    real(kind=rb) :: z(nlay+2,ncomp)
    real(kind=rb) :: svar_f, svar_s, svar_i, svar_f_bnd(jpband), svar_s_bnd(jpband), svar_i_bnd(jpband)
    real(kind=rb), parameter :: zepzen = 1.e-10_rb
    icld = icld_in; iaer = iaer_in
    if (icld.lt.0.or.icld.gt.3) icld = 2
    if (iaer.ne.0.and.iaer.ne.6.and.iaer.ne.10) iaer = 0
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
      call spcvrt_sw(nlayers, jpb1, jpb2, 1, 1, 0, pavel, tavel, pz, tz, tbound, albdif, albdir, &
           cldfrac, ztauc, zasyc, zomgc, ztaucorig, ztaua, zasya, zomga, cossza, coldry, wkl, adjflux, &
           isolvar, svar_f, svar_s, svar_i, svar_f_bnd, svar_s_bnd, svar_i_bnd, &
           laytrop, layswtch, laylow, jp, jt, jt1, co2mult, colch4, colco2, colh2o, colmol, coln2o, colo2, colo3, &
           fac00, fac01, fac10, fac11, selffac, selffrac, indself, forfac, forfrac, indfor, &
           z(:,2), z(:,1), z(:,4), z(:,3), z(:,7), z(:,8), z(:,11), z(:,12), &
           z(:,5), z(:,6), z(:,9), z(:,10), z(:,13), z(:,14))
      do i = 1, nlayers+1
        swuflxc(iplon,i) = z(i,3)
        swdflxc(iplon,i) = z(i,4)
        swuflx(iplon,i) = z(i,1)
        swdflx(iplon,i) = z(i,2)
      enddo
      do i = 1, nlayers+1
        swnflxc(i) = swdflxc(iplon,i) - swuflxc(iplon,i)
        swnflx(i) = swdflx(iplon,i) - swuflx(iplon,i)
      enddo
      do i = 1, nlayers
        zdpgcp = heatfac / pdp(i)
        swhrc(iplon,i) = (swnflxc(i+1) - swnflxc(i)) * zdpgcp
        swhr(iplon,i) = (swnflx(i+1) - swnflx(i)) * zdpgcp
      enddo
    enddo
  end subroutine sw_albedo_nomcica

  subroutine sw_albedo_mcica(ncol, nlay, icld_in, iaer_in, play, plev, tlay, tlev, tsfc, &
      h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, albdir_in, albdif_in, coszen, adjes, dyofyr, scon, isolvar, &
      inflgsw, iceflgsw, liqflgsw, cldfmcl, taucmcl, ssacmcl, asmcmcl, fsfcmcl, ciwpmcl, clwpmcl, reicmcl, relqmcl, &
      tauaer, ssaaer, asmaer, bndsolvar, indsolvar, solcycfrac, &
      swuflx, swdflx, swhr, swuflxc, swdflxc, swhrc) bind(c)
    use rrtmg_sw_rad, only : inatm_sw
    use rrtmg_sw_cldprmc, only : cldprmc_sw
    use rrtmg_sw_setcoef, only : setcoef_sw
    use rrtmg_sw_spcvmc, only : spcvmc_sw
    use rrsw_con, only : heatfac
    integer(kind=im), intent(in) :: ncol, nlay, icld_in, iaer_in, dyofyr, isolvar, inflgsw, iceflgsw, liqflgsw
    real(kind=rb), intent(in) :: play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol)
    real(kind=rb), intent(in) :: h2ovmr(ncol,nlay), o3vmr(ncol,nlay), co2vmr(ncol,nlay), ch4vmr(ncol,nlay), n2ovmr(ncol,nlay), o2vmr(ncol,nlay)
    real(kind=rb), intent(in) :: albdir_in(ncol,nbndsw), albdif_in(ncol,nbndsw), coszen(ncol), adjes, scon, solcycfrac
    real(kind=rb), intent(in) :: cldfmcl(ngptsw,ncol,nlay), taucmcl(ngptsw,ncol,nlay), ssacmcl(ngptsw,ncol,nlay)
    real(kind=rb), intent(in) :: asmcmcl(ngptsw,ncol,nlay), fsfcmcl(ngptsw,ncol,nlay), ciwpmcl(ngptsw,ncol,nlay), clwpmcl(ngptsw,ncol,nlay)
    real(kind=rb), intent(in) :: reicmcl(ncol,nlay), relqmcl(ncol,nlay)
    real(kind=rb), intent(in) :: tauaer(ncol,nlay,nbndsw), ssaaer(ncol,nlay,nbndsw), asmaer(ncol,nlay,nbndsw)
    real(kind=rb), intent(in) :: bndsolvar(nbndsw)
    real(kind=rb), intent(inout) :: indsolvar(2)
    real(kind=rb), intent(out) :: swuflx(ncol,nlay+1), swdflx(ncol,nlay+1), swhr(ncol,nlay), swuflxc(ncol,nlay+1), swdflxc(ncol,nlay+1), swhrc(ncol,nlay)
    real(kind=rb) :: swnflx(nlay+2), swnflxc(nlay+2), zdpgcp
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
    real(kind=rb) :: z(nlay+2,ncomp)
    real(kind=rb) :: svar_f, svar_s, svar_i, svar_f_bnd(jpband), svar_s_bnd(jpband), svar_i_bnd(jpband)
    real(kind=rb), parameter :: zepzen = 1.e-10_rb
    icld = icld_in; iaer = iaer_in
    if (icld.lt.0.or.icld.gt.3) icld = 2
    if (iaer.ne.0.and.iaer.ne.6.and.iaer.ne.10) iaer = 0
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
      call spcvmc_sw(nlayers, jpb1, jpb2, 1, 1, 0, pavel, tavel, pz, tz, tbound, albdif, albdir, &
           zcldfmc, ztaucmc, zasycmc, zomgcmc, ztaormc, ztaua, zasya, zomga, cossza, coldry, wkl, adjflux, &
           isolvar, svar_f, svar_s, svar_i, svar_f_bnd, svar_s_bnd, svar_i_bnd, &
           laytrop, layswtch, laylow, jp, jt, jt1, co2mult, colch4, colco2, colh2o, colmol, coln2o, colo2, colo3, &
           fac00, fac01, fac10, fac11, selffac, selffrac, indself, forfac, forfrac, indfor, &
           z(:,2), z(:,1), z(:,4), z(:,3), z(:,7), z(:,8), z(:,11), z(:,12), &
           z(:,5), z(:,6), z(:,9), z(:,10), z(:,13), z(:,14))
      do i = 1, nlayers+1
        swuflxc(iplon,i) = z(i,3)
        swdflxc(iplon,i) = z(i,4)
        swuflx(iplon,i) = z(i,1)
        swdflx(iplon,i) = z(i,2)
      enddo
      do i = 1, nlayers+1
        swnflxc(i) = swdflxc(iplon,i) - swuflxc(iplon,i)
        swnflx(i) = swdflx(iplon,i) - swuflx(iplon,i)
      enddo
      do i = 1, nlayers
        zdpgcp = heatfac / pdp(i)
        swhrc(iplon,i) = (swnflxc(i+1) - swnflxc(i)) * zdpgcp
        swhr(iplon,i) = (swnflx(i+1) - swnflx(i)) * zdpgcp
      enddo
    enddo
  end subroutine sw_albedo_mcica
end module sw_albedo_shim
