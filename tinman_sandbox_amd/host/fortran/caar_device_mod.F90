! caar_device_mod.F90 -- Fortran (iso_c_binding) interface for a host whose element arrays live on the device in
! Fortran order (include/caar_f90.h): compute_and_apply_rhs runs on them in place, no layout conversion, no second copy.
!
! Binds caar_launch_f90 / caar_launch_steps_f90, the library's device allocator (caar_arrays_alloc / caar_arrays_free:
! the 16 buffers are the same size in both orders, so they hold Fortran-ordered arrays as they are), and the few HIP runtime
! calls such a host needs, the way hipfort binds them.  The types are caar_mod's (include/caar.h).
module caar_device_mod
  use iso_c_binding
  use caar_mod, only: caar_dims_t, caar_arrays_t, caar_params_t
  implicit none
  public

  ! hipMemcpyKind (hip_runtime_api.h)
  integer(c_int), parameter :: hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2

  interface
    ! one compute_and_apply_rhs on Fortran-ordered DEVICE arrays; dvv_dev: np*np doubles on the device, row-major
    integer(c_int) function caar_launch_f90(dims, f90_dev, dvv_dev, prm, stream) bind(C, name="caar_launch_f90")
      import; type(caar_dims_t) :: dims; type(caar_arrays_t) :: f90_dev; type(c_ptr), value :: dvv_dev
      type(caar_params_t) :: prm; type(c_ptr), value :: stream
    end function
    ! nsteps of them, with update_time_levels in between if rotate /= 0
    integer(c_int) function caar_launch_steps_f90(dims, f90_dev, dvv_dev, prm, nsteps, rotate, stream) &
        bind(C, name="caar_launch_steps_f90")
      import; type(caar_dims_t) :: dims; type(caar_arrays_t) :: f90_dev; type(c_ptr), value :: dvv_dev
      type(caar_params_t) :: prm; integer(c_int), value :: nsteps, rotate; type(c_ptr), value :: stream
    end function
    integer(c_int) function caar_arrays_alloc(arena, dims, device, out_dev) bind(C, name="caar_arrays_alloc")
      import; type(c_ptr) :: arena; type(caar_dims_t) :: dims; integer(c_int), value :: device
      type(caar_arrays_t) :: out_dev
    end function
    integer(c_int) function caar_arrays_free(arena) bind(C, name="caar_arrays_free")
      import; type(c_ptr), value :: arena
    end function
    ! HIP runtime
    integer(c_int) function hipMalloc(ptr, bytes) bind(C, name="hipMalloc")
      import; type(c_ptr) :: ptr; integer(c_size_t), value :: bytes
    end function
    integer(c_int) function hipFree(ptr) bind(C, name="hipFree")
      import; type(c_ptr), value :: ptr
    end function
    integer(c_int) function hipMemcpy(dst, src, bytes, kind) bind(C, name="hipMemcpy")
      import; type(c_ptr), value :: dst, src; integer(c_size_t), value :: bytes; integer(c_int), value :: kind
    end function
    integer(c_int) function hipDeviceSynchronize() bind(C, name="hipDeviceSynchronize")
      import
    end function
  end interface

end module caar_device_mod
