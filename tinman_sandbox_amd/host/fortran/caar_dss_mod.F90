! caar_dss_mod.F90 -- Fortran (iso_c_binding) interface of the direct stiffness summation of the new time level
! (include/caar_dss.h): what edgeVpack / bndry_exchangeV / edgeVunpack and the rspheremp multiply do for the elements one
! device holds, on T, v and dp3d at one time level, in place.
!
! A HOMME host passes its gdofP(np,np,nelemd) as integer(c_long_long) with layout = CAAR_DSS_LAYOUT_F90, and launches on the
! Fortran-ordered device arrays of caar_device_mod with rspheremp(np,np,nelemd) on the device.  The types are caar_mod's
! (include/caar.h).  One DSS may be in flight per plan: the plan owns its edge buffer.
module caar_dss_mod
  use iso_c_binding
  use caar_mod, only: caar_dims_t, caar_arrays_t
  implicit none
  public

  integer(c_int), parameter :: CAAR_DSS_MAX_SHARERS = 8
  integer(c_int), parameter :: CAAR_DSS_LAYOUT_CXX = 0, CAAR_DSS_LAYOUT_F90 = 1

  interface
    ! sharer lists of gdof_host (HOST, np*np*num_elems ids) built on the host, uploaded to `device` (< 0: host-only plan)
    integer(c_int) function caar_dss_plan_create(plan, dims, gdof_host, layout, device) bind(C, name="caar_dss_plan_create")
      import; type(c_ptr) :: plan; type(caar_dims_t) :: dims; integer(c_long_long) :: gdof_host(*)
      integer(c_int), value :: layout, device
    end function
    subroutine caar_dss_plan_destroy(plan) bind(C, name="caar_dss_plan_destroy")
      import; type(c_ptr), value :: plan
    end subroutine
    integer(c_int) function caar_dss_plan_info(plan, unique_points, shared_points, open_points, max_sharers) &
        bind(C, name="caar_dss_plan_info")
      import; type(c_ptr), value :: plan; integer(c_long_long) :: unique_points, shared_points, open_points
      integer(c_int) :: max_sharers
    end function
    ! one DSS of T, v, dp3d at time level tl (0-based) of DEVICE arrays; rspheremp_dev: np*np*num_elems doubles on the device
    integer(c_int) function caar_dss_launch(plan, dims, layout, arrays_dev, tl, rspheremp_dev, stream) &
        bind(C, name="caar_dss_launch")
      import; type(c_ptr), value :: plan; type(caar_dims_t) :: dims; integer(c_int), value :: layout
      type(caar_arrays_t) :: arrays_dev; integer(c_int), value :: tl; type(c_ptr), value :: rspheremp_dev, stream
    end function
  end interface

end module caar_dss_mod
