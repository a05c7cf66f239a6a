! caar_f90_resident.F90 -- a Fortran host whose element arrays stay on the MI355X in Fortran order.
!
! The reference Fortran driver's state (compute_and_apply_rhs_test/fortran/main.F90: closed-form initialisation :103-154
! with the single-precision Dvv literals :83-96, the same as caar_f90_driver.F90) is copied up ONCE, as it is, into buffers
! from the library's allocator (caar_arrays_alloc); then `loopmax` calls of caar_launch_f90 run on it in place -- no layout
! conversion, no second copy -- and the state comes back once for the reference's norm lines (main.F90:168-194, 278-304)
! and one `ms per call` line.  argv(1) = number of elements (default 3), argv(2) = loopmax (default 10000, kinds.F90).
program caar_f90_resident
  use iso_c_binding
  use caar_mod, only: caar_dims_t, caar_arrays_t, caar_params_t, caar_device_count, caar_check
  use caar_device_mod
  implicit none
  integer, parameter :: np = 4, nlev = 72, qsize_d = 1, timelevels = 3
  integer :: nelemd = 3, loopmax = 10000
  real(c_double), allocatable, target :: D(:,:,:,:,:), Dinv(:,:,:,:,:)
  real(c_double), allocatable, target :: fcor(:,:,:), spheremp(:,:,:), metdet(:,:,:), rmetdet(:,:,:), phis(:,:,:)
  real(c_double), allocatable, target :: dp3d(:,:,:,:,:), v(:,:,:,:,:,:), T(:,:,:,:,:), Qdp(:,:,:,:,:,:)
  real(c_double), allocatable, target :: eta_dot_dpdn(:,:,:,:), omega_p(:,:,:,:), phi(:,:,:,:), pecnd(:,:,:,:)
  real(c_double), allocatable, target :: vn0(:,:,:,:,:)
  real(c_double), target :: Dvv_c(np*np)
  real(c_double) :: Dvv(np,np)
  real(c_double) :: gi(np,np), gj(np,np), zk, ze
  real, parameter :: dvv_single(np*np) = (/ -3.0, -0.80901699437494745, 0.30901699437494745, -0.5, &
      4.0450849718747373, 0.0, -1.1180339887498949, 1.5450849718747370, &
      -1.5450849718747370, 1.1180339887498949, 0.0, -4.0450849718747373, &
      0.5, -0.30901699437494745, 0.80901699437494745, 3.0 /)
  type(caar_dims_t) :: dims
  type(caar_arrays_t) :: h, dv   ! host / device pointers (Fortran names ignore case: not `d`, D is an array)
  type(caar_params_t) :: prm
  type(c_ptr) :: arena, dvv_dev
  integer :: i, j, k, ie, tl, it
  integer(c_int) :: rc
  integer(8) :: t0, t1, rate
  character(len=32) :: arg

  if (command_argument_count() >= 1) then
    call get_command_argument(1, arg)
    read (arg, *) nelemd
  end if
  if (command_argument_count() >= 2) then
    call get_command_argument(2, arg)
    read (arg, *) loopmax
  end if
  print *, "Main: nelemd = ", nelemd
  if (caar_device_count() < 1) then
    print *, "No HIP device is visible: the MI355X path cannot run (there is no CPU fallback)."
    error stop 1
  end if

  allocate(D(np,np,2,2,nelemd), Dinv(np,np,2,2,nelemd))
  allocate(fcor(np,np,nelemd), spheremp(np,np,nelemd), metdet(np,np,nelemd), rmetdet(np,np,nelemd), phis(np,np,nelemd))
  allocate(dp3d(np,np,nlev,timelevels,nelemd), v(np,np,2,nlev,timelevels,nelemd), T(np,np,nlev,timelevels,nelemd))
  allocate(Qdp(np,np,nlev,qsize_d,2,nelemd))
  allocate(eta_dot_dpdn(np,np,nlev+1,nelemd), omega_p(np,np,nlev,nelemd), phi(np,np,nlev,nelemd), pecnd(np,np,nlev,nelemd))
  allocate(vn0(np,np,2,nlev,nelemd))

  ! Derivative matrix: DEFAULT-REAL literals widened to double (main.F90:83-96), as in caar_f90_driver.F90; the C ABI
  ! wants row-major Dvv[i][j]
  Dvv = real(reshape(dvv_single, (/ np, np /)), c_double)
  Dvv_c = reshape(transpose(Dvv), (/ np*np /))

  ! Closed-form fields of the reference driver (main.F90:103-154), the expressions of caar_f90_driver.F90
  gi = spread((/ (real(i, c_double), i = 1, np) /), dim=2, ncopies=np)
  gj = spread((/ (real(j, c_double), j = 1, np) /), dim=1, ncopies=np)
  D = 0
  Dinv = 0
  eta_dot_dpdn = 0
  Qdp = 0
  vn0 = 1.0
  pecnd = 1.0
  do ie = 1, nelemd
    ze = ie
    fcor(:,:,ie) = sin(gi + gj)
    metdet(:,:,ie) = gi*gj
    rmetdet(:,:,ie) = 1.0d0/metdet(:,:,ie)
    spheremp(:,:,ie) = 2*gi
    phis(:,:,ie) = gi + gj
    D(:,:,1,1,ie) = 1.0
    D(:,:,2,2,ie) = 2.0
    Dinv(:,:,1,1,ie) = 1.0
    Dinv(:,:,2,2,ie) = 0.5
    do k = 1, nlev
      zk = k
      phi(:,:,k,ie) = cos(gi + 3*gj) + zk
      omega_p(:,:,k,ie) = gj*gj
      Qdp(:,:,k,1,1,ie) = 1.0 + sin(gi*gj*zk)
      do tl = 1, timelevels
        dp3d(:,:,k,tl,ie) = 10*zk + ze + gi + gj + tl
        v(:,:,1,k,tl,ie) = 1.0 + zk/2 + gi + gj + ze/5 + tl*2.0
        v(:,:,2,k,tl,ie) = 1.0 + zk/2 + gi + gj + ze/5 + tl*3.0
        T(:,:,k,tl,ie) = 1000 - zk - gi - gj + ze/10 + tl
      end do
    end do
  end do

  call print_norms()   ! the np1 state before the calls (main.F90:168-194)
  print *, 'Main, np=', np

  dims%np = np; dims%nlev = nlev; dims%qsize_d = qsize_d; dims%timelevels = timelevels; dims%num_elems = nelemd
  h%elem_D = c_loc(D); h%elem_Dinv = c_loc(Dinv); h%elem_fcor = c_loc(fcor); h%elem_spheremp = c_loc(spheremp)
  h%elem_metdet = c_loc(metdet); h%elem_rmetdet = c_loc(rmetdet)
  h%elem_state_dp3d = c_loc(dp3d); h%elem_state_v = c_loc(v); h%elem_state_T = c_loc(T)
  h%elem_state_phis = c_loc(phis); h%elem_state_Qdp = c_loc(Qdp)
  h%elem_derived_eta_dot_dpdn = c_loc(eta_dot_dpdn); h%elem_derived_omega_p = c_loc(omega_p)
  h%elem_derived_phi = c_loc(phi); h%elem_derived_pecnd = c_loc(pecnd); h%elem_derived_vn0 = c_loc(vn0)

  ! device buffers from the library's allocator, filled once with the Fortran-ordered arrays as they are
  call caar_check(caar_arrays_alloc(arena, dims, 0_c_int, dv), 'caar_arrays_alloc')
  call hip_check(hipMemcpy(dv%elem_D, h%elem_D, nbytes(size(D)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_Dinv, h%elem_Dinv, nbytes(size(Dinv)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_fcor, h%elem_fcor, nbytes(size(fcor)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_spheremp, h%elem_spheremp, nbytes(size(spheremp)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_metdet, h%elem_metdet, nbytes(size(metdet)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_rmetdet, h%elem_rmetdet, nbytes(size(rmetdet)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_state_dp3d, h%elem_state_dp3d, nbytes(size(dp3d)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_state_v, h%elem_state_v, nbytes(size(v)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_state_T, h%elem_state_T, nbytes(size(T)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_state_phis, h%elem_state_phis, nbytes(size(phis)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_state_Qdp, h%elem_state_Qdp, nbytes(size(Qdp)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_derived_eta_dot_dpdn, h%elem_derived_eta_dot_dpdn, nbytes(size(eta_dot_dpdn)), &
                           hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_derived_omega_p, h%elem_derived_omega_p, nbytes(size(omega_p)), hipMemcpyHostToDevice), &
                 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_derived_phi, h%elem_derived_phi, nbytes(size(phi)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_derived_pecnd, h%elem_derived_pecnd, nbytes(size(pecnd)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMemcpy(dv%elem_derived_vn0, h%elem_derived_vn0, nbytes(size(vn0)), hipMemcpyHostToDevice), 'hipMemcpy')
  call hip_check(hipMalloc(dvv_dev, nbytes(size(Dvv_c))), 'hipMalloc')
  call hip_check(hipMemcpy(dvv_dev, c_loc(Dvv_c), nbytes(size(Dvv_c)), hipMemcpyHostToDevice), 'hipMemcpy')

  ! the reference's 1-based (np1,nm1,n0,qn0) = (2,3,1,1) and elements nets..nete = 1..nelemd
  prm%nets = 0; prm%nete = nelemd; prm%n0 = 0; prm%np1 = 1; prm%nm1 = 2; prm%qn0 = 0
  prm%dt2 = 1.0d0; prm%eta_ave_w = 1.0d0
  prm%rrearth = 1.0d0/6.376d6; prm%Rwater_vapor = 461.5d0; prm%Rgas = 287.04d0; prm%kappa = 287.04d0/1005.0d0
  prm%ps0 = 10.0d0; prm%hyai0 = nlev + 1          ! hvcoord%hyai(1) = nlev + 2 - 1 (main.F90:160-162)
  prm%Dvv = c_loc(Dvv_c)

  ! the reference's loop (main.F90:201-210): loopmax calls on the same time levels, here on the device-resident state
  call hip_check(hipDeviceSynchronize(), 'hipDeviceSynchronize')
  call system_clock(t0, rate)
  do it = 1, loopmax
    rc = caar_launch_f90(dims, dv, dvv_dev, prm, c_null_ptr)   ! == call compute_and_apply_rhs(...)
    call caar_check(rc, 'caar_launch_f90')
  end do
  call hip_check(hipDeviceSynchronize(), 'hipDeviceSynchronize')
  call system_clock(t1)

  ! the state back, once
  call hip_check(hipMemcpy(h%elem_state_dp3d, dv%elem_state_dp3d, nbytes(size(dp3d)), hipMemcpyDeviceToHost), 'hipMemcpy')
  call hip_check(hipMemcpy(h%elem_state_v, dv%elem_state_v, nbytes(size(v)), hipMemcpyDeviceToHost), 'hipMemcpy')
  call hip_check(hipMemcpy(h%elem_state_T, dv%elem_state_T, nbytes(size(T)), hipMemcpyDeviceToHost), 'hipMemcpy')
  call print_norms()   ! after the calls (main.F90:278-304)
  print '(a, f12.6)', ' ms per call = ', 1.0d3 * real(t1 - t0, c_double) / real(rate, c_double) / max(loopmax, 1)
  call hip_check(hipFree(dvv_dev), 'hipFree')
  call caar_check(caar_arrays_free(arena), 'caar_arrays_free')

contains

  integer(c_size_t) function nbytes(n)   ! of n doubles
    integer, intent(in) :: n
    nbytes = int(n, c_size_t) * 8_c_size_t
  end function

  subroutine hip_check(e, what)
    integer(c_int), intent(in) :: e
    character(len=*), intent(in) :: what
    if (e /= 0) then
      print *, 'hip: ', what, ' failed with code ', e
      error stop 1
    end if
  end subroutine

  ! ||x||_2 with the squares summed in order and the rounding error of each addition carried along (Kahan)
  real(c_double) function kahan_norm(x, n)
    integer, intent(in) :: n
    real(c_double), intent(in) :: x(n)
    real(c_double) :: s, c, y, t
    integer :: m
    s = 0; c = 0
    do m = 1, n
      y = x(m)*x(m) - c
      t = s + y
      c = (t - s) - y
      s = t
    end do
    kahan_norm = sqrt(s)
  end function

  ! the reference's three norm lines for time level np1: per-element norms, then the norm over the elements
  subroutine print_norms()
    real(c_double) :: vn(nelemd), tn(nelemd), dn(nelemd)
    integer :: e
    do e = 1, nelemd
      vn(e) = kahan_norm(reshape(v(:,:,:,:,2,e), (/ np*np*2*nlev /)), np*np*2*nlev)
      tn(e) = kahan_norm(reshape(T(:,:,:,2,e), (/ np*np*nlev /)), np*np*nlev)
      dn(e) = kahan_norm(reshape(dp3d(:,:,:,2,e), (/ np*np*nlev /)), np*np*nlev)
    end do
    print *, "||v||_2  = ", kahan_norm(vn, nelemd)
    print *, "||T||_2  = ", kahan_norm(tn, nelemd)
    print *, "||dp||_2 = ", kahan_norm(dn, nelemd)
  end subroutine

end program caar_f90_resident
