!======================================================================!
MODULE H9_GPU
!----------------------------------------------------------------------!
! ISO_C_BINDING interface of libh9g.so (include/h9g.h): the Fortran side
! of the drop-in boundary.  A HYBRID9 host replaces the cell loop of
! /root/reference/SOURCE/HYBRID9.f90:120-295 by one h9g_run_year call per
! simulated year (see INTEGRATION.md).  Arrays are passed by reference
! with the SHARED.f90 layouts: per-layer (L,ncell) layer-fastest,
! per-cell (ncell), forcing (ncell,nday) per variable stacked as
! (ncell,nday,7) in READ_PGF.f90 order tas rlds rsds huss ps pr rhs.
!----------------------------------------------------------------------!
USE, INTRINSIC :: ISO_C_BINDING
IMPLICIT NONE

INTEGER, PARAMETER :: H9G_LMAX = 10
INTEGER, PARAMETER :: H9G_NDIAG = 12
INTEGER, PARAMETER :: H9G_NDAILY = 11
INTEGER, PARAMETER :: H9G_NMONTHS = 12
INTEGER, PARAMETER :: H9G_NDAYREC = 7
INTEGER, PARAMETER :: H9G_ERR_TRIDIAG1 = 1, H9G_ERR_TRIDIAG2 = 2
INTEGER, PARAMETER :: H9G_ERR_RSUB_POS = 3, H9G_ERR_IMBALANCE = 4
INTEGER, PARAMETER :: H9G_ERR_NOSNAP = 5   ! internal invariant, not a reference STOP

TYPE, BIND(C) :: h9g_config
  INTEGER(C_INT32_T) :: ncell, nlayers, nisurf, grow_on, max_days, nslots
  REAL(C_FLOAT) :: zi (0:H9G_LMAX+1)
END TYPE h9g_config

TYPE, BIND(C) :: h9g_error
  INTEGER(C_INT32_T) :: code, cell, year, day, substep
  REAL(C_FLOAT) :: value
END TYPE h9g_error

! h9g_spinup's options (include/h9g.h): a cell settles at cycle k >=
! min_cycles once its column water (mm), water table (mm) and relative
! plant-mass drifts over a cycle are within the tolerances.
INTEGER, PARAMETER :: H9G_NSPIN = 6
TYPE, BIND(C) :: h9g_spinup_opts
  INTEGER(C_INT32_T) :: max_cycles, min_cycles, freeze, reserved
  REAL(C_DOUBLE) :: tol_water, tol_zwt, tol_plant
END TYPE h9g_spinup_opts

! h9g_get_daystats' thresholds (include/h9g.h): a runoff day has q >= q_thr
! (mm/day), a dry day theta(1) < theta_thr, a wet day zwt <= zwt_thr (mm), a
! green day LAI >= lai_thr; reserved = 0.
INTEGER, PARAMETER :: H9G_NDAYSTAT = 17
TYPE, BIND(C) :: h9g_daystat_opts
  REAL(C_FLOAT) :: q_thr, theta_thr, zwt_thr, lai_thr
  INTEGER(C_INT32_T) :: reserved (4)
END TYPE h9g_daystat_opts

! h9g_get_dayquant's options (include/h9g.h): series 0: q, 1: e, 2..6: record
! rows 2..6; nq probabilities p in [0, 1] (hydrology's Q95 is p = 0.05);
! pooled = 1: one result over all years of the span; reserved = 0.
INTEGER, PARAMETER :: H9G_NQUANT_MAX = 16
TYPE, BIND(C) :: h9g_dayquant_opts
  INTEGER(C_INT32_T) :: series, nq, pooled, reserved
  REAL(C_DOUBLE) :: p (H9G_NQUANT_MAX)
END TYPE h9g_dayquant_opts

INTERFACE
  ! Day statistics of years k0 .. k0+nk-1 (0-based) of the last run that
  ! recorded days, reduced on the device: out (ncell, 17, nk).
  FUNCTION h9g_get_daystats (ctx, k0, nk, opts, out) BIND(C, NAME='h9g_get_daystats')
    IMPORT :: C_PTR, C_INT, C_DOUBLE, h9g_daystat_opts
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: k0, nk
    TYPE(h9g_daystat_opts), INTENT(IN) :: opts
    REAL(C_DOUBLE), INTENT(OUT) :: out (*)
    INTEGER(C_INT) :: h9g_get_daystats
  END FUNCTION
  ! Device ms of the last h9g_get_daystats' launches.
  FUNCTION h9g_last_daystat_ms (ctx) BIND(C, NAME='h9g_last_daystat_ms')
    IMPORT :: C_PTR, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    REAL(C_FLOAT) :: h9g_last_daystat_ms
  END FUNCTION
  ! The same kernel on hand-made records (n, 7, nt), nseg slices a year
  ! (0: the product's): out (n, 17).
  FUNCTION h9g_daystat_selftest (device, n, nt, nseg, records, opts, out) &
           BIND(C, NAME='h9g_daystat_selftest')
    IMPORT :: C_INT, C_FLOAT, C_DOUBLE, h9g_daystat_opts
    INTEGER(C_INT), VALUE :: device, n, nt, nseg
    REAL(C_FLOAT), INTENT(IN) :: records (*)
    TYPE(h9g_daystat_opts), INTENT(IN) :: opts
    REAL(C_DOUBLE), INTENT(OUT) :: out (*)
    INTEGER(C_INT) :: h9g_daystat_selftest
  END FUNCTION
  ! One year of day statistics (ncell, 17) to sxyYYYY.nc: 17 float64
  ! variables on axyYYYY.nc's grid, the thresholds as global attributes.
  FUNCTION h9g_write_sxy_nc (path, nx, ny, ncell, gid, jyear, opts, stats) &
           BIND(C, NAME='h9g_write_sxy_nc')
    IMPORT :: C_INT, C_CHAR, C_DOUBLE, C_INT64_T, h9g_daystat_opts
    CHARACTER(KIND=C_CHAR), INTENT(IN) :: path (*)
    INTEGER(C_INT), VALUE :: nx, ny, ncell, jyear
    INTEGER(C_INT64_T), INTENT(IN) :: gid (*)
    TYPE(h9g_daystat_opts), INTENT(IN) :: opts
    REAL(C_DOUBLE), INTENT(IN) :: stats (*)
    INTEGER(C_INT) :: h9g_write_sxy_nc
  END FUNCTION
  ! Order statistics of one daily series of years k0 .. k0+nk-1 (0-based) of
  ! the last run that recorded days, selected on the device: out (ncell,
  ! 1 + 2 nq, nres), nres = 1 when opts%pooled = 1, else nk.
  FUNCTION h9g_get_dayquant (ctx, k0, nk, opts, out) BIND(C, NAME='h9g_get_dayquant')
    IMPORT :: C_PTR, C_INT, C_DOUBLE, h9g_dayquant_opts
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: k0, nk
    TYPE(h9g_dayquant_opts), INTENT(IN) :: opts
    REAL(C_DOUBLE), INTENT(OUT) :: out (*)
    INTEGER(C_INT) :: h9g_get_dayquant
  END FUNCTION
  ! Device ms of the last h9g_get_dayquant's launches.
  FUNCTION h9g_last_dayquant_ms (ctx) BIND(C, NAME='h9g_last_dayquant_ms')
    IMPORT :: C_PTR, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    REAL(C_FLOAT) :: h9g_last_dayquant_ms
  END FUNCTION
  ! The same kernel on hand-made records (n, 7, ntmax, nyears) of nt(y) days a
  ! year, nseg slices a year (0: the product's): out (n, 1 + 2 nq, nres).
  FUNCTION h9g_dayquant_selftest (device, n, nyears, nt, nseg, records, opts, out) &
           BIND(C, NAME='h9g_dayquant_selftest')
    IMPORT :: C_INT, C_INT32_T, C_FLOAT, C_DOUBLE, h9g_dayquant_opts
    INTEGER(C_INT), VALUE :: device, n, nyears, nseg
    INTEGER(C_INT32_T), INTENT(IN) :: nt (*)
    REAL(C_FLOAT), INTENT(IN) :: records (*)
    TYPE(h9g_dayquant_opts), INTENT(IN) :: opts
    REAL(C_DOUBLE), INTENT(OUT) :: out (*)
    INTEGER(C_INT) :: h9g_dayquant_selftest
  END FUNCTION
  ! One result of h9g_get_dayquant (ncell, 1 + 2 nq) to qxyYYYY.nc (or
  ! qxyYYYY_YYYY.nc): count, lower, upper and the interpolated value per
  ! quantile on axyYYYY.nc's grid, the series and years as global attributes.
  FUNCTION h9g_write_qxy_nc (path, nx, ny, ncell, gid, year_first, year_last, opts, quant) &
           BIND(C, NAME='h9g_write_qxy_nc')
    IMPORT :: C_INT, C_CHAR, C_DOUBLE, C_INT64_T, h9g_dayquant_opts
    CHARACTER(KIND=C_CHAR), INTENT(IN) :: path (*)
    INTEGER(C_INT), VALUE :: nx, ny, ncell, year_first, year_last
    INTEGER(C_INT64_T), INTENT(IN) :: gid (*)
    TYPE(h9g_dayquant_opts), INTENT(IN) :: opts
    REAL(C_DOUBLE), INTENT(IN) :: quant (*)
    INTEGER(C_INT) :: h9g_write_qxy_nc
  END FUNCTION
  ! Spin-up to equilibrium: years jyear0 .. jyear0+nyears-1 (isolated cells,
  ! the forcing of year jyear0+k resident in slots(k+1)) repeated until the
  ! cells settle; history (H9G_NSPIN, max_cycles).
  FUNCTION h9g_spinup (ctx, slots, jyear0, nyears, opts, cycles_run, cell_cycle, history) &
           BIND(C, NAME='h9g_spinup')
    IMPORT :: C_PTR, C_INT, C_INT32_T, C_DOUBLE, h9g_spinup_opts
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT32_T), INTENT(IN) :: slots (*)
    INTEGER(C_INT), VALUE :: jyear0, nyears
    TYPE(h9g_spinup_opts), INTENT(IN) :: opts
    INTEGER(C_INT32_T), INTENT(OUT) :: cycles_run
    INTEGER(C_INT32_T), INTENT(OUT) :: cell_cycle (*)
    REAL(C_DOUBLE), INTENT(OUT) :: history (*)
    INTEGER(C_INT) :: h9g_spinup
  END FUNCTION
  FUNCTION h9g_spin_selftest (device, n, L, state_prev, state, err, opts, k, list, &
                              cell_cycle, stats) BIND(C, NAME='h9g_spin_selftest')
    IMPORT :: C_INT, C_INT32_T, C_FLOAT, C_DOUBLE, h9g_spinup_opts
    INTEGER(C_INT), VALUE :: device, n, L, k
    REAL(C_FLOAT), INTENT(IN) :: state_prev (*), state (*)
    INTEGER(C_INT32_T), INTENT(IN) :: err (*)
    TYPE(h9g_spinup_opts), INTENT(IN) :: opts
    INTEGER(C_INT32_T), INTENT(OUT) :: list (*), cell_cycle (*)
    REAL(C_DOUBLE), INTENT(OUT) :: stats (*)
    INTEGER(C_INT) :: h9g_spin_selftest
  END FUNCTION
  FUNCTION h9g_abi_version () BIND(C, NAME='h9g_abi_version')
    IMPORT :: C_INT
    INTEGER(C_INT) :: h9g_abi_version
  END FUNCTION
  FUNCTION h9g_device_count () BIND(C, NAME='h9g_device_count')
    IMPORT :: C_INT
    INTEGER(C_INT) :: h9g_device_count
  END FUNCTION
  FUNCTION h9g_create (cfg, device) BIND(C, NAME='h9g_create')
    IMPORT :: C_PTR, C_INT, h9g_config
    TYPE(h9g_config), INTENT(IN) :: cfg
    INTEGER(C_INT), VALUE :: device
    TYPE(C_PTR) :: h9g_create
  END FUNCTION
  FUNCTION h9g_config_check (cfg, reason, reason_len) BIND(C, NAME='h9g_config_check')
    IMPORT :: C_INT, C_CHAR, h9g_config
    TYPE(h9g_config), INTENT(IN) :: cfg
    CHARACTER(KIND=C_CHAR), INTENT(OUT) :: reason (*)
    INTEGER(C_INT), VALUE :: reason_len
    INTEGER(C_INT) :: h9g_config_check
  END FUNCTION
  FUNCTION h9g_config_bytes (cfg) BIND(C, NAME='h9g_config_bytes')
    IMPORT :: C_SIZE_T, h9g_config
    TYPE(h9g_config), INTENT(IN) :: cfg
    INTEGER(C_SIZE_T) :: h9g_config_bytes
  END FUNCTION
  FUNCTION h9g_create_error () BIND(C, NAME='h9g_create_error')
    IMPORT :: C_PTR
    TYPE(C_PTR) :: h9g_create_error
  END FUNCTION
  FUNCTION h9g_build_id () BIND(C, NAME='h9g_build_id')
    IMPORT :: C_PTR
    TYPE(C_PTR) :: h9g_build_id
  END FUNCTION
  SUBROUTINE h9g_destroy (ctx) BIND(C, NAME='h9g_destroy')
    IMPORT :: C_PTR
    TYPE(C_PTR), VALUE :: ctx
  END SUBROUTINE
  FUNCTION h9g_set_params (ctx, theta_s, hksat, bsw, psi_s, fmax) &
           BIND(C, NAME='h9g_set_params')
    IMPORT :: C_PTR, C_INT, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    REAL(C_FLOAT), INTENT(IN) :: theta_s (*), hksat (*), bsw (*), psi_s (*), fmax (*)
    INTEGER(C_INT) :: h9g_set_params
  END FUNCTION
  FUNCTION h9g_init_state (ctx) BIND(C, NAME='h9g_init_state')
    IMPORT :: C_PTR, C_INT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT) :: h9g_init_state
  END FUNCTION
  FUNCTION h9g_state_size (nlayers) BIND(C, NAME='h9g_state_size')
    IMPORT :: C_INT
    INTEGER(C_INT), VALUE :: nlayers
    INTEGER(C_INT) :: h9g_state_size
  END FUNCTION
  FUNCTION h9g_set_state (ctx, packed) BIND(C, NAME='h9g_set_state')
    IMPORT :: C_PTR, C_INT, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    REAL(C_FLOAT), INTENT(IN) :: packed (*)
    INTEGER(C_INT) :: h9g_set_state
  END FUNCTION
  FUNCTION h9g_get_state (ctx, packed) BIND(C, NAME='h9g_get_state')
    IMPORT :: C_PTR, C_INT, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    REAL(C_FLOAT), INTENT(OUT) :: packed (*)
    INTEGER(C_INT) :: h9g_get_state
  END FUNCTION
  FUNCTION h9g_push_forcing (ctx, slot, nday, forcing, async) &
           BIND(C, NAME='h9g_push_forcing')
    IMPORT :: C_PTR, C_INT, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: slot, nday, async
    REAL(C_FLOAT), INTENT(IN) :: forcing (*)
    INTEGER(C_INT) :: h9g_push_forcing
  END FUNCTION
  FUNCTION h9g_push_forcing_device (ctx, slot, nday, dev) &
           BIND(C, NAME='h9g_push_forcing_device')
    IMPORT :: C_PTR, C_INT
    TYPE(C_PTR), VALUE :: ctx, dev
    INTEGER(C_INT), VALUE :: slot, nday
    INTEGER(C_INT) :: h9g_push_forcing_device
  END FUNCTION
  FUNCTION h9g_forcing_slot (ctx, slot) BIND(C, NAME='h9g_forcing_slot')
    IMPORT :: C_PTR, C_INT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: slot
    TYPE(C_PTR) :: h9g_forcing_slot
  END FUNCTION
  FUNCTION h9g_host_alloc (bytes) BIND(C, NAME='h9g_host_alloc')
    IMPORT :: C_PTR, C_SIZE_T
    INTEGER(C_SIZE_T), VALUE :: bytes
    TYPE(C_PTR) :: h9g_host_alloc
  END FUNCTION
  SUBROUTINE h9g_host_free (p) BIND(C, NAME='h9g_host_free')
    IMPORT :: C_PTR
    TYPE(C_PTR), VALUE :: p
  END SUBROUTINE
  FUNCTION h9g_run_year (ctx, slot, jyear) BIND(C, NAME='h9g_run_year')
    IMPORT :: C_PTR, C_INT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: slot, jyear
    INTEGER(C_INT) :: h9g_run_year
  END FUNCTION
  FUNCTION h9g_sync (ctx) BIND(C, NAME='h9g_sync')
    IMPORT :: C_PTR, C_INT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT) :: h9g_sync
  END FUNCTION
  FUNCTION h9g_last_error (ctx, err) BIND(C, NAME='h9g_last_error')
    IMPORT :: C_PTR, C_INT, h9g_error
    TYPE(C_PTR), VALUE :: ctx
    TYPE(h9g_error), INTENT(OUT) :: err
    INTEGER(C_INT) :: h9g_last_error
  END FUNCTION
  FUNCTION h9g_get_annual (ctx, annual) BIND(C, NAME='h9g_get_annual')
    IMPORT :: C_PTR, C_INT, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    REAL(C_FLOAT), INTENT(OUT) :: annual (*)
    INTEGER(C_INT) :: h9g_get_annual
  END FUNCTION
  FUNCTION h9g_get_diagnostics (ctx, host_out, dev_out) &
           BIND(C, NAME='h9g_get_diagnostics')
    IMPORT :: C_PTR, C_INT, C_DOUBLE
    TYPE(C_PTR), VALUE :: ctx, dev_out
    REAL(C_DOUBLE), INTENT(OUT) :: host_out (*)
    INTEGER(C_INT) :: h9g_get_diagnostics
  END FUNCTION
  FUNCTION h9g_get_errors (ctx, rec) BIND(C, NAME='h9g_get_errors')
    IMPORT :: C_PTR, C_INT, C_INT32_T
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT32_T), INTENT(OUT) :: rec (*)
    INTEGER(C_INT) :: h9g_get_errors
  END FUNCTION
  ! The reference's cell order over one decade (HYBRID9.f90:93-130: smp
  ! carried from cell to cell); annual (ncell, 12+L, nyears) in C order
  ! (nyears, 12+L, ncell).
  FUNCTION h9g_run_decade_ordered (ctx, slots, jyear0, nyears, annual, passes) &
           BIND(C, NAME='h9g_run_decade_ordered')
    IMPORT :: C_PTR, C_INT, C_INT32_T, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT32_T), INTENT(IN) :: slots (*)
    INTEGER(C_INT), VALUE :: jyear0, nyears
    REAL(C_FLOAT), INTENT(OUT) :: annual (*)
    INTEGER(C_INT32_T), INTENT(OUT) :: passes
    INTEGER(C_INT) :: h9g_run_decade_ordered
  END FUNCTION
  ! The same over several decades at once (every year's forcing resident),
  ! the decades overlapping on the device; passes: one per decade.
  FUNCTION h9g_run_ordered (ctx, slots, jyear0, nyears, annual, passes) &
           BIND(C, NAME='h9g_run_ordered')
    IMPORT :: C_PTR, C_INT, C_INT32_T, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT32_T), INTENT(IN) :: slots (*)
    INTEGER(C_INT), VALUE :: jyear0, nyears
    REAL(C_FLOAT), INTENT(OUT) :: annual (*)
    INTEGER(C_INT32_T), INTENT(OUT) :: passes (*)
    INTEGER(C_INT) :: h9g_run_ordered
  END FUNCTION
  FUNCTION h9g_ordered_stats (ctx, out, n) BIND(C, NAME='h9g_ordered_stats')
    IMPORT :: C_PTR, C_INT, C_INT64_T
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT64_T), INTENT(OUT) :: out (*)
    INTEGER(C_INT), VALUE :: n
    INTEGER(C_INT) :: h9g_ordered_stats
  END FUNCTION
  FUNCTION h9g_set_chains (ctx, chain) BIND(C, NAME='h9g_set_chains')
    IMPORT :: C_PTR, C_INT, C_INT32_T
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT32_T), INTENT(IN) :: chain (*)
    INTEGER(C_INT) :: h9g_set_chains
  END FUNCTION
  FUNCTION h9g_decade_stats (ctx, out, n) BIND(C, NAME='h9g_decade_stats')
    IMPORT :: C_PTR, C_INT, C_INT64_T
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT64_T), INTENT(OUT) :: out (*)
    INTEGER(C_INT), VALUE :: n
    INTEGER(C_INT) :: h9g_decade_stats
  END FUNCTION
  FUNCTION h9g_get_diagnostics_async (ctx, dev_out, stream) &
           BIND(C, NAME='h9g_get_diagnostics_async')
    IMPORT :: C_PTR, C_INT
    TYPE(C_PTR), VALUE :: ctx, dev_out, stream
    INTEGER(C_INT) :: h9g_get_diagnostics_async
  END FUNCTION
  FUNCTION h9g_set_cells (ctx, gid, lat) BIND(C, NAME='h9g_set_cells')
    IMPORT :: C_PTR, C_INT, C_INT64_T, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT64_T), INTENT(IN) :: gid (*)
    REAL(C_FLOAT), INTENT(IN) :: lat (*)
    INTEGER(C_INT) :: h9g_set_cells
  END FUNCTION
  FUNCTION h9g_synth_params (ctx, seed) BIND(C, NAME='h9g_synth_params')
    IMPORT :: C_PTR, C_INT, C_INT64_T
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT64_T), VALUE :: seed
    INTEGER(C_INT) :: h9g_synth_params
  END FUNCTION
  FUNCTION h9g_synth_forcing (ctx, slot, seed, day0, nday) &
           BIND(C, NAME='h9g_synth_forcing')
    IMPORT :: C_PTR, C_INT, C_INT64_T
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: slot, day0, nday
    INTEGER(C_INT64_T), VALUE :: seed
    INTEGER(C_INT) :: h9g_synth_forcing
  END FUNCTION
  FUNCTION h9g_land_cells (nx, ny, nland, seed, gid, lat) &
           BIND(C, NAME='h9g_land_cells')
    IMPORT :: C_INT, C_INT64_T, C_FLOAT
    INTEGER(C_INT), VALUE :: nx, ny, nland
    INTEGER(C_INT64_T), VALUE :: seed
    INTEGER(C_INT64_T), INTENT(OUT) :: gid (*)
    REAL(C_FLOAT), INTENT(OUT) :: lat (*)
    INTEGER(C_INT) :: h9g_land_cells
  END FUNCTION
  ! NetCDF I/O (h9g_io.cpp): WRITE_NET_CDF_3DR.f90 / READ_PGF.f90
  FUNCTION h9g_write_axy_nc (path, nx, ny, nlayers, zc, ncell, gid, annual) &
      BIND(C, NAME='h9g_write_axy_nc')
    IMPORT :: C_INT, C_CHAR, C_FLOAT, C_INT64_T
    CHARACTER(KIND=C_CHAR), INTENT(IN) :: path (*)
    INTEGER(C_INT), VALUE :: nx, ny, nlayers, ncell
    REAL(C_FLOAT), INTENT(IN) :: zc (*), annual (*)
    INTEGER(C_INT64_T), INTENT(IN) :: gid (*)
    INTEGER(C_INT) :: h9g_write_axy_nc
  END FUNCTION
  FUNCTION h9g_nc_forcing_read (paths, nx, ny, ncell, gid, t0, nt, out) &
      BIND(C, NAME='h9g_nc_forcing_read')
    IMPORT :: C_INT, C_PTR, C_FLOAT, C_INT64_T
    TYPE(C_PTR), INTENT(IN) :: paths (*)
    INTEGER(C_INT), VALUE :: nx, ny, ncell, t0, nt
    INTEGER(C_INT64_T), INTENT(IN) :: gid (*)
    REAL(C_FLOAT) :: out (*)
    INTEGER(C_INT) :: h9g_nc_forcing_read
  END FUNCTION
  FUNCTION h9g_nc_ntimes (path) BIND(C, NAME='h9g_nc_ntimes')
    IMPORT :: C_INT, C_CHAR
    CHARACTER(KIND=C_CHAR), INTENT(IN) :: path (*)
    INTEGER(C_INT) :: h9g_nc_ntimes
  END FUNCTION
  FUNCTION h9g_nc_read_stats (out, n) BIND(C, NAME='h9g_nc_read_stats')
    IMPORT :: C_INT, C_DOUBLE
    REAL(C_DOUBLE), INTENT(OUT) :: out (*)
    INTEGER(C_INT), VALUE :: n
    INTEGER(C_INT) :: h9g_nc_read_stats
  END FUNCTION
  FUNCTION h9g_nc_forcing_prefetch (ctx, slot, paths, nx, ny, t0, nt) &
      BIND(C, NAME='h9g_nc_forcing_prefetch')
    IMPORT :: C_INT, C_PTR
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: slot, nx, ny, t0, nt
    TYPE(C_PTR), INTENT(IN) :: paths (*)
    INTEGER(C_INT) :: h9g_nc_forcing_prefetch
  END FUNCTION
  ! soil parameter build (INIT.f90:492-680)
  FUNCTION h9g_soil_layer (ctx, layer, ts, ks, lm, ps, nx, ny, on_device) &
      BIND(C, NAME='h9g_soil_layer')
    IMPORT :: C_INT, C_PTR, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: layer, nx, ny, on_device
    REAL(C_FLOAT), INTENT(IN) :: ts (*), ks (*), lm (*), ps (*)
    INTEGER(C_INT) :: h9g_soil_layer
  END FUNCTION
  FUNCTION h9g_soil_fmax (ctx, soil_tex, fmax, nx, ny) BIND(C, NAME='h9g_soil_fmax')
    IMPORT :: C_INT, C_PTR, C_INT32_T
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT32_T), INTENT(IN) :: soil_tex (*), fmax (*)
    INTEGER(C_INT), VALUE :: nx, ny
    INTEGER(C_INT) :: h9g_soil_fmax
  END FUNCTION
  FUNCTION h9g_last_soil_ms (ctx) BIND(C, NAME='h9g_last_soil_ms')
    IMPORT :: C_PTR, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    REAL(C_FLOAT) :: h9g_last_soil_ms
  END FUNCTION
  FUNCTION h9g_last_soil_slow (ctx) BIND(C, NAME='h9g_last_soil_slow')
    IMPORT :: C_PTR, C_INT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT) :: h9g_last_soil_slow
  END FUNCTION
  FUNCTION h9g_get_params (ctx, theta_s, hksat, bsw, psi_s, fmax) BIND(C, NAME='h9g_get_params')
    IMPORT :: C_INT, C_PTR, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    REAL(C_FLOAT) :: theta_s (*), hksat (*), bsw (*), psi_s (*), fmax (*)
    INTEGER(C_INT) :: h9g_get_params
  END FUNCTION
  ! LCLIM single-site path (HYBRID9.f90:339-480): sub (cells, 5, nday*NISURF),
  ! daily (cells, 2, nday), lai (cells, 3, nday), diag (cells, 11, nday)
  FUNCTION h9g_run_site (ctx, nday, sub, daily, lai, diag) BIND(C, NAME='h9g_run_site')
    IMPORT :: C_INT, C_PTR, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: nday
    REAL(C_FLOAT) :: sub (*), daily (*), lai (*), diag (*)
    INTEGER(C_INT) :: h9g_run_site
  END FUNCTION
  ! Daily diagnostics of selected cells (HYBRID9.f90:221-229): cells(nsel)
  ! are 0-based context indices, strictly increasing; nsel = 0 turns it off.
  FUNCTION h9g_set_daily (ctx, nsel, cells) BIND(C, NAME='h9g_set_daily')
    IMPORT :: C_PTR, C_INT, C_INT32_T
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: nsel
    INTEGER(C_INT32_T), INTENT(IN) :: cells (*)
    INTEGER(C_INT) :: h9g_set_daily
  END FUNCTION
  ! The lines of year k (0-based) of the last run: out (nsel, 11, nday_k).
  FUNCTION h9g_get_daily (ctx, k, out) BIND(C, NAME='h9g_get_daily')
    IMPORT :: C_PTR, C_INT, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: k
    REAL(C_FLOAT) :: out (*)
    INTEGER(C_INT) :: h9g_get_daily
  END FUNCTION
  ! Monthly output: on /= 0 makes later runs record the year's 12+L running
  ! sums at every month end (the monthly year kernels); 0 (default) turns it off.
  FUNCTION h9g_set_monthly (ctx, on) BIND(C, NAME='h9g_set_monthly')
    IMPORT :: C_PTR, C_INT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: on
    INTEGER(C_INT) :: h9g_set_monthly
  END FUNCTION
  ! The snapshots of year k (0-based) of the last run: out (ncell, 12+L, 12).
  FUNCTION h9g_get_monthly (ctx, k, out) BIND(C, NAME='h9g_get_monthly')
    IMPORT :: C_PTR, C_INT, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: k
    REAL(C_FLOAT) :: out (*)
    INTEGER(C_INT) :: h9g_get_monthly
  END FUNCTION
  ! Monthly means of year jyear from its snapshots (ncell, 12+L, 12) to
  ! mxyYYYY.nc: the fields of h9g_write_axy_nc under a leading dimension month.
  FUNCTION h9g_write_mxy_nc (path, nx, ny, nlayers, zc, ncell, gid, jyear, nisurf, snapshots) &
      BIND(C, NAME='h9g_write_mxy_nc')
    IMPORT :: C_INT, C_CHAR, C_FLOAT, C_INT64_T
    CHARACTER(KIND=C_CHAR), INTENT(IN) :: path (*)
    INTEGER(C_INT), VALUE :: nx, ny, nlayers, ncell, jyear, nisurf
    REAL(C_FLOAT), INTENT(IN) :: zc (*), snapshots (*)
    INTEGER(C_INT64_T), INTENT(IN) :: gid (*)
    INTEGER(C_INT) :: h9g_write_mxy_nc
  END FUNCTION
  ! The same file from the snapshots of an ET run (h9g_set_evap): evaporation
  ! divided by days_m * nisurf, like runoff.
  FUNCTION h9g_write_mxy_nc_evap (path, nx, ny, nlayers, zc, ncell, gid, jyear, nisurf, snapshots) &
      BIND(C, NAME='h9g_write_mxy_nc_evap')
    IMPORT :: C_INT, C_CHAR, C_FLOAT, C_INT64_T
    CHARACTER(KIND=C_CHAR), INTENT(IN) :: path (*)
    INTEGER(C_INT), VALUE :: nx, ny, nlayers, ncell, jyear, nisurf
    REAL(C_FLOAT), INTENT(IN) :: zc (*), snapshots (*)
    INTEGER(C_INT64_T), INTENT(IN) :: gid (*)
    INTEGER(C_INT) :: h9g_write_mxy_nc_evap
  END FUNCTION
  ! Evapotranspiration output: on /= 0 makes later runs use the ET year
  ! kernels, whose row evap of the annual means and of the month-end snapshots
  ! is the year's evaporation sum; 0 (default): the reference's zero.
  FUNCTION h9g_set_evap (ctx, on) BIND(C, NAME='h9g_set_evap')
    IMPORT :: C_PTR, C_INT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: on
    INTEGER(C_INT) :: h9g_set_evap
  END FUNCTION
  ! Day records: on /= 0 makes later runs use the day year kernels, which
  ! store 7 values per cell and day; needs h9g_set_evap on (H9G_ESTATE else).
  FUNCTION h9g_set_days (ctx, on) BIND(C, NAME='h9g_set_days')
    IMPORT :: C_PTR, C_INT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: on
    INTEGER(C_INT) :: h9g_set_days
  END FUNCTION
  ! The records of year k (0-based) of the last run: out (ncell, 7, nday_k).
  FUNCTION h9g_get_days (ctx, k, out) BIND(C, NAME='h9g_get_days')
    IMPORT :: C_PTR, C_INT, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: k
    REAL(C_FLOAT) :: out (*)
    INTEGER(C_INT) :: h9g_get_days
  END FUNCTION
  ! One year of day records (ncell, 7, nday) to dxyYYYY.nc: seven variables
  ! under a leading dimension time, runoff and evapotranspiration per day.
  FUNCTION h9g_write_dxy_nc (path, nx, ny, nlayers, zc, ncell, gid, jyear, nday, records) &
      BIND(C, NAME='h9g_write_dxy_nc')
    IMPORT :: C_INT, C_CHAR, C_FLOAT, C_INT64_T
    CHARACTER(KIND=C_CHAR), INTENT(IN) :: path (*)
    INTEGER(C_INT), VALUE :: nx, ny, nlayers, ncell, jyear, nday
    REAL(C_FLOAT), INTENT(IN) :: zc (*), records (*)
    INTEGER(C_INT64_T), INTENT(IN) :: gid (*)
    INTEGER(C_INT) :: h9g_write_dxy_nc
  END FUNCTION
  FUNCTION h9g_last_kernel_ms (ctx) BIND(C, NAME='h9g_last_kernel_ms')
    IMPORT :: C_PTR, C_FLOAT
    TYPE(C_PTR), VALUE :: ctx
    REAL(C_FLOAT) :: h9g_last_kernel_ms
  END FUNCTION
  FUNCTION h9g_total_kernel_ms (ctx, reset) BIND(C, NAME='h9g_total_kernel_ms')
    IMPORT :: C_PTR, C_INT, C_DOUBLE
    TYPE(C_PTR), VALUE :: ctx
    INTEGER(C_INT), VALUE :: reset
    REAL(C_DOUBLE) :: h9g_total_kernel_ms
  END FUNCTION
  FUNCTION h9g_launch_stats (ctx, out, n, reset) BIND(C, NAME='h9g_launch_stats')
    IMPORT :: C_PTR, C_INT, C_DOUBLE
    TYPE(C_PTR), VALUE :: ctx
    REAL(C_DOUBLE), INTENT(OUT) :: out (*)
    INTEGER(C_INT), VALUE :: n, reset
    INTEGER(C_INT) :: h9g_launch_stats
  END FUNCTION
END INTERFACE

CONTAINS

  !--------------------------------------------------------------------!
  ! Print the reference's STOP diagnostics for the first failing cell
  ! and stop, as HYDROLOGY.f90:806-825,1068-1072,1244-1274 do.
  !--------------------------------------------------------------------!
  SUBROUTINE h9g_check_stop (ctx, rc)
    TYPE(C_PTR), INTENT(IN) :: ctx
    INTEGER(C_INT), INTENT(IN) :: rc
    TYPE(h9g_error) :: e
    INTEGER(C_INT) :: r
    IF (rc == 0) RETURN
    IF (rc < 0) THEN
      WRITE (*,*) 'h9g API/HIP failure, code ', rc
      STOP 'h9g failure'
    END IF
    r = h9g_last_error (ctx, e)
    SELECT CASE (e%code)
    CASE (H9G_ERR_TRIDIAG1)
      WRITE (*,*) 'Problem with tridiagonal 1.'
    CASE (H9G_ERR_TRIDIAG2)
      WRITE (*,*) 'Problem with tridiagonal 2.'
    CASE (H9G_ERR_RSUB_POS)
      WRITE (*,*) 'rsub_top_tot is positive in drainage'
      WRITE (*,*) 'HYBRID9 is stopping'
    CASE (H9G_ERR_NOSNAP)
      WRITE (*,*) 'h9g internal: exact re-run with no day snapshot'
    CASE DEFAULT
      WRITE (*,*) 'Problem in HYDROLOGY'
      WRITE (*,*) 'Water imbalance > 0.1 mm ', e%value
    END SELECT
    WRITE (*,*) 'DiTIME = ', e%day + 1
    WRITE (*,*) 'cell year substep ', e%cell + 1, e%year, e%substep + 1
    STOP
  END SUBROUTINE h9g_check_stop

END MODULE H9_GPU
!======================================================================!
