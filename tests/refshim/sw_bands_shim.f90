! TEST INFRASTRUCTURE ONLY.  Our own bind(c) driver around the REFERENCE's shortwave module procedures, for the fluxes BY
! BAND: the reference's spcvrt_sw / spcvmc_sw take a band range (istart, iend) and restart their g-point counter at the
! band when iout > 0, but its driver pins them to all bands.  Per column and in driver order it calls inatm_sw -> cldprop_sw
! (cldprmc_sw on McICA sub-columns) -> setcoef_sw -> the iaer 0 / 10 aerosol copy, as rrtmg_sw_rad.nomcica.f90:587-794 and
! rrtmg_sw_rad.f90:616-819 do, and then spcvrt_sw (spcvmc_sw) once over the full range (iout = 0: slot 0, checked against the
! binder's outputs bit for bit) and once per band with istart = iend = iout = band (slots 1..14 = bands 16..29).  Compiled
! against the reference's .mod files and linked against its shared library by tests/refshim/build_bands.sh (see
! sw_components_shim.f90, whose driver steps these are).
!
! Arguments follow rrtmg_sw_{nomcica,mcica}_wrapper of the binder (iaer 6 is not supported here).  Output:
! bands(ncol, nlay+1, 6, 0:14), level 1 = surface, the six sums in this order: zbbfu zbbfd zbbcu zbbcd zbbfddir zbbcddir.
module sw_bands_shim
  use iso_c_binding
  use parkind, only : im => kind_im, rb => kind_rb
  use parrrsw, only : nbndsw, ngptsw, mxmol, jpband, jpb1, jpb2
  implicit none
  integer, parameter :: ncomp = 14, nout = 6
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

  subroutine albedos(iplon, ncol, asdir, asdif, aldir, aldif, albdir, albdif)
    integer(kind=im), intent(in) :: iplon, ncol
    real(kind=rb), intent(in) :: asdir(ncol), asdif(ncol), aldir(ncol), aldif(ncol)
    real(kind=rb), intent(out) :: albdir(nbndsw), albdif(nbndsw)
    albdir(1:9) = aldir(iplon); albdif(1:9) = aldif(iplon)
    albdir(nbndsw) = aldir(iplon); albdif(nbndsw) = aldif(iplon)
    albdir(10:13) = asdir(iplon); albdif(10:13) = asdif(iplon)
  end subroutine albedos

  subroutine sw_bands_nomcica(ncol, nlay, icld_in, iaer_in, play, plev, tlay, tlev, tsfc, &
      h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, asdir, asdif, aldir, aldif, coszen, adjes, dyofyr, scon, isolvar, &
      inflgsw, iceflgsw, liqflgsw, cldfr, taucld, ssacld, asmcld, fsfcld, cicewp, cliqwp, reice, reliq, &
      tauaer, ssaaer, asmaer, bndsolvar, indsolvar, solcycfrac, bands) bind(c)
    use rrtmg_sw_rad_nomcica, only : inatm_sw
    use rrtmg_sw_cldprop, only : cldprop_sw
    use rrtmg_sw_setcoef, only : setcoef_sw
    use rrtmg_sw_spcvrt, only : spcvrt_sw
    integer(kind=im), intent(in) :: ncol, nlay, icld_in, iaer_in, dyofyr, isolvar, inflgsw, iceflgsw, liqflgsw
    real(kind=rb), intent(in) :: play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol)
    real(kind=rb), intent(in) :: h2ovmr(ncol,nlay), o3vmr(ncol,nlay), co2vmr(ncol,nlay), ch4vmr(ncol,nlay), n2ovmr(ncol,nlay), o2vmr(ncol,nlay)
    real(kind=rb), intent(in) :: asdir(ncol), asdif(ncol), aldir(ncol), aldif(ncol), coszen(ncol), adjes, scon, solcycfrac
    real(kind=rb), intent(in) :: cldfr(ncol,nlay)
    real(kind=rb), intent(in) :: taucld(nbndsw,ncol,nlay), ssacld(nbndsw,ncol,nlay), asmcld(nbndsw,ncol,nlay), fsfcld(nbndsw,ncol,nlay)
    real(kind=rb), intent(in) :: cicewp(ncol,nlay), cliqwp(ncol,nlay), reice(ncol,nlay), reliq(ncol,nlay)
    real(kind=rb), intent(in) :: tauaer(ncol,nlay,nbndsw), ssaaer(ncol,nlay,nbndsw), asmaer(ncol,nlay,nbndsw)
    real(kind=rb), intent(in) :: bndsolvar(nbndsw)
    real(kind=rb), intent(inout) :: indsolvar(2)
    real(kind=rb), intent(out) :: bands(ncol,nlay+1,nout,0:nbndsw)
    integer(kind=im) :: kb, i1, i2, io
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
      call albedos(iplon, ncol, asdir, asdif, aldir, aldif, albdir, albdif)
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
      do kb = 0, nbndsw
        if (kb .eq. 0) then
          i1 = jpb1; i2 = jpb2; io = 0
        else
          i1 = jpb1-1+kb; i2 = i1; io = i1
        endif
        z = 0._rb
        call spcvrt_sw(nlayers, i1, i2, 1, 1, io, pavel, tavel, pz, tz, tbound, albdif, albdir, &
             cldfrac, ztauc, zasyc, zomgc, ztaucorig, ztaua, zasya, zomga, cossza, coldry, wkl, adjflux, &
             isolvar, svar_f, svar_s, svar_i, svar_f_bnd, svar_s_bnd, svar_i_bnd, &
             laytrop, layswtch, laylow, jp, jt, jt1, co2mult, colch4, colco2, colh2o, colmol, coln2o, colo2, colo3, &
             fac00, fac01, fac10, fac11, selffac, selffrac, indself, forfac, forfrac, indfor, &
             z(:,2), z(:,1), z(:,4), z(:,3), z(:,7), z(:,8), z(:,11), z(:,12), &
             z(:,5), z(:,6), z(:,9), z(:,10), z(:,13), z(:,14))
        bands(iplon,:,:,kb) = z(1:nlay+1,1:nout)
      enddo
    enddo
  end subroutine sw_bands_nomcica

  subroutine sw_bands_mcica(ncol, nlay, icld_in, iaer_in, play, plev, tlay, tlev, tsfc, &
      h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, asdir, asdif, aldir, aldif, coszen, adjes, dyofyr, scon, isolvar, &
      inflgsw, iceflgsw, liqflgsw, cldfmcl, taucmcl, ssacmcl, asmcmcl, fsfcmcl, ciwpmcl, clwpmcl, reicmcl, relqmcl, &
      tauaer, ssaaer, asmaer, bndsolvar, indsolvar, solcycfrac, bands) bind(c)
    use rrtmg_sw_rad, only : inatm_sw
    use rrtmg_sw_cldprmc, only : cldprmc_sw
    use rrtmg_sw_setcoef, only : setcoef_sw
    use rrtmg_sw_spcvmc, only : spcvmc_sw
    integer(kind=im), intent(in) :: ncol, nlay, icld_in, iaer_in, dyofyr, isolvar, inflgsw, iceflgsw, liqflgsw
    real(kind=rb), intent(in) :: play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol)
    real(kind=rb), intent(in) :: h2ovmr(ncol,nlay), o3vmr(ncol,nlay), co2vmr(ncol,nlay), ch4vmr(ncol,nlay), n2ovmr(ncol,nlay), o2vmr(ncol,nlay)
    real(kind=rb), intent(in) :: asdir(ncol), asdif(ncol), aldir(ncol), aldif(ncol), coszen(ncol), adjes, scon, solcycfrac
    real(kind=rb), intent(in) :: cldfmcl(ngptsw,ncol,nlay), taucmcl(ngptsw,ncol,nlay), ssacmcl(ngptsw,ncol,nlay)
    real(kind=rb), intent(in) :: asmcmcl(ngptsw,ncol,nlay), fsfcmcl(ngptsw,ncol,nlay), ciwpmcl(ngptsw,ncol,nlay), clwpmcl(ngptsw,ncol,nlay)
    real(kind=rb), intent(in) :: reicmcl(ncol,nlay), relqmcl(ncol,nlay)
    real(kind=rb), intent(in) :: tauaer(ncol,nlay,nbndsw), ssaaer(ncol,nlay,nbndsw), asmaer(ncol,nlay,nbndsw)
    real(kind=rb), intent(in) :: bndsolvar(nbndsw)
    real(kind=rb), intent(inout) :: indsolvar(2)
    real(kind=rb), intent(out) :: bands(ncol,nlay+1,nout,0:nbndsw)
    integer(kind=im) :: kb, i1, i2, io
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
      call albedos(iplon, ncol, asdir, asdif, aldir, aldif, albdir, albdif)
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
      do kb = 0, nbndsw
        if (kb .eq. 0) then
          i1 = jpb1; i2 = jpb2; io = 0
        else
          i1 = jpb1-1+kb; i2 = i1; io = i1
        endif
        z = 0._rb
        call spcvmc_sw(nlayers, i1, i2, 1, 1, io, pavel, tavel, pz, tz, tbound, albdif, albdir, &
             zcldfmc, ztaucmc, zasycmc, zomgcmc, ztaormc, ztaua, zasya, zomga, cossza, coldry, wkl, adjflux, &
             isolvar, svar_f, svar_s, svar_i, svar_f_bnd, svar_s_bnd, svar_i_bnd, &
             laytrop, layswtch, laylow, jp, jt, jt1, co2mult, colch4, colco2, colh2o, colmol, coln2o, colo2, colo3, &
             fac00, fac01, fac10, fac11, selffac, selffrac, indself, forfac, forfrac, indfor, &
             z(:,2), z(:,1), z(:,4), z(:,3), z(:,7), z(:,8), z(:,11), z(:,12), &
             z(:,5), z(:,6), z(:,9), z(:,10), z(:,13), z(:,14))
        bands(iplon,:,:,kb) = z(1:nlay+1,1:nout)
      enddo
    enddo
  end subroutine sw_bands_mcica
end module sw_bands_shim
