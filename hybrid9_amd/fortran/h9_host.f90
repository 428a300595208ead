!======================================================================!
PROGRAM H9_HOST
!----------------------------------------------------------------------!
! MI355X host driver for HYBRID9's per-cell hot path.
!
! Restates the PGF path of /root/reference/SOURCE/HYBRID9.f90:81-333 with
! the cell loop (:120-295) replaced by the GPU: one h9g_run_year per
! simulated year advances every land cell (all days x NISURF substeps of
! HYDROLOGY, daily GROW), then the annual means (axy_*, :263-290) come
! back with h9g_get_annual.  Configuration keeps the reference surface:
! driver.txt is read with the same list-directed sequence as
! INIT.f90:181-204.  Inputs, since NetCDF/PGF/BNU are unavailable here:
!   input_mode = 'synth' : synthetic 0.5/0.25 deg land grid generated on
!                          the device (hybrid9_amd/synth.py bit-for-bit)
!   input_mode = 'case'  : a raw case directory (params.f32, forcing.f32,
!                          optional state0.f32, case.nml) -- the same files
!                          the reference harness oracle/_ref/h9ref reads
!   input_mode = 'pgf'   : forcing from the 7 PGF NetCDF files per decade
!                          (READ_PGF.f90 names <var>_pgfv2.1_<syr>_<eyr>.nc4
!                          in pgf_dir, netCDF classic), read on a host
!                          thread and copied while the previous year runs
!                          (h9g_nc_forcing_prefetch); synthetic soil
! chosen in the optional namelist file h9gpu.nml (/h9gpu/); nx, ny, nland
! override the synthetic grid.
!
! cell_order = 1 (default) runs the reference's own order: decade by
! decade (HYBRID9.f90:93-130), each land cell's first substep of a decade
! reading the smp its predecessor in (y, x) order left behind (HYDROLOGY.
! f90:270-275, SHARED.f90:198), through h9g_run_ordered -- bit for bit the
! reference on one rank.  Every year of a call is staged into its own slot
! and the call overlaps its decades on the device; ordered_decades > 0 cuts
! the run into calls of that many decades (HBM: 0.69 GB per 0.5 deg year),
! 0 (default) makes one call.  cell_order = 0: every cell its own smp
! (h9g_run_year per year, isolated-cell semantics, DESIGN.md §1).
!
! daily = 1 records the daily diagnostics line (HYBRID9.f90:221-229) of
! every cell of the run (h9g_set_daily, DESIGN.md §7) and writes them to
! <out_dir>/daily.f32 as (ncell, 11, total days); the cell order then runs
! decade by decade through h9g_run_decade_ordered.  INTERACTIVE = .T. in
! driver.txt, on a grid (synth/pgf), is the reference's focus window
! (INIT.f90:220-236, 280-283, 462-466): the land list is cut to the window
! of lon_c_w x lat_c_w cells from (lon_w, lat_w), all of them recorded, and
! LCLIM/daily_diag.csv is written under the working directory with the
! reference's header, format and order (decade, cell, year, day).
!
! monthly = 1 records every year kernel's month-end running sums
! (h9g_set_monthly, DESIGN.md §7) and writes each year's monthly means to
! <out_dir>/mxyYYYY.nc (h9g_write_mxy_nc: axyYYYY.nc's fields under a leading
! dimension month), in both cell_order settings; ordered_decades is left as
! given (the decades stay overlapped).  On a grid the cells sit at their grid
! ids; a case's cells form a grid of one row, in their order.
!
! evap = 1 turns evapotranspiration recording on (h9g_set_evap, DESIGN.md §7):
! the evaporation field of axyYYYY.nc, of annual.f32 and, with monthly = 1, of
! mxyYYYY.nc (then written by h9g_write_mxy_nc_evap) is the year's evaporation
! sum instead of the reference's zero, in both cell_order settings.
!
! days = 1 records every year kernel's day-end records (h9g_set_days,
! DESIGN.md §7: runoff and ET sums, column water, top-layer water content,
! water table, aquifer water and LAI of every cell on every day) and writes
! each year's to <out_dir>/dxyYYYY.nc (h9g_write_dxy_nc), in both cell_order
! settings and with or without monthly; it implies evap = 1.  The grid is
! mxyYYYY.nc's.
!
! daystats = 1 reduces every year's day records on the device to 17 numbers per
! cell (h9g_get_daystats, DESIGN.md §7: the largest daily runoff and its day,
! the lowest 7-day flow, the driest the column got, the longest dry spell, ...)
! with the thresholds q_thr (mm/day), theta_thr, zwt_thr (mm) and lai_thr, and
! writes each year's to <out_dir>/sxyYYYY.nc (h9g_write_sxy_nc) where
! dxyYYYY.nc is written, in both cell_order settings; it implies days and evap.
! The dxy file is then written only if days = 1 was set too.
!
! dayquant = 1 selects order statistics of one daily series on the device
! (h9g_get_dayquant, DESIGN.md §7: the flow-duration curve, the median water
! table, ...): quant_series (0: q, 1: e, 2..6: record rows 2..6; default 0) at
! the probabilities quant_p (up to 16, each in [0, 1]; unset entries are -1;
! default 0.05, 0.5, 0.95 -- hydrology's Q95 is p = 0.05), and writes each
! year's to <out_dir>/qxyYYYY.nc (h9g_write_qxy_nc), in both cell_order
! settings; it implies days and evap like daystats.  quant_pool = 1 pools the
! years of every ordered call instead (cell_order = 1 only: an isolated run
! retains one year) and writes <out_dir>/qxyYYYY_YYYY.nc per call.
!
! spinup_cycles > 0 (0 = off, the default) spins the cold start of
! INIT.f90:707-811 up to equilibrium before the run proper (h9g_spinup,
! DESIGN.md §7): the run's first spinup_years years (default 1) are staged
! into their own slots and repeated, isolated cells, at most spinup_cycles
! times; a cell settles at a cycle >= spinup_min_cycles (default 1) once its
! column water and water table drifts over a cycle are within spinup_tol_water
! and spinup_tol_zwt (mm) and its relative plant-mass drift within
! spinup_tol_plant (defaults: a huge value, criterion off); spinup_freeze = 1
! (default) takes a settled cell out of the later cycles.  In either
! cell_order setting: spin-up only produces the start state of the run proper,
! whose years are unchanged.  Writes <out_dir>/spinup.txt, one line per cycle
! (cycle, cells run, settled, stopped, the maxima of the three drifts), and
! <out_dir>/spinup_cycle.i32 (ncell int32: the cycle each cell settled at, 0
! still active, -1 never ran, -2 stopped).  A STOP during spin-up ends the
! program after both files are written.
!
! Usage:  h9_host [driver.txt] [h9gpu.nml]
! Outputs: <out_dir>/annual.f32 (ncell, 12+L, nyears),
!          <out_dir>/state_end.f32 (packed state, include/h9g.h) and, on a
!          grid (synth/pgf), <PATH_output>/axyYYYY.nc per year as
!          HYBRID9.f90:492-519 / WRITE_NET_CDF_3DR.f90 (nc_out = 1).
!----------------------------------------------------------------------!
USE, INTRINSIC :: ISO_C_BINDING
USE H9_GPU
IMPLICIT NONE

! --- driver.txt (INIT.f90:181-204) ---------------------------------------
CHARACTER (LEN = 200) :: PATH_output, LCLIM_filename, LSOIL_filename
INTEGER :: NISURF, iDEC_start, iDEC_end, syr, eyr, NYR_SPIN_UP
LOGICAL :: PGF, INTERACTIVE, LCLIM
REAL :: lon_w, lat_w, lon_c_w, lat_c_w
REAL(C_FLOAT) :: zi (0:H9G_LMAX+1)

! --- extension namelist ----------------------------------------------------
CHARACTER (LEN = 512) :: input_mode, case_dir, out_dir, pgf_dir
INTEGER :: nlayers, grow_on, device, grid, year0, nyears, nc_out, gnx, gny, gnland
INTEGER :: cell_order, ordered_decades, daily, monthly, evap, days, daystats
INTEGER :: dayquant, quant_series, quant_pool
REAL(C_DOUBLE) :: quant_p (H9G_NQUANT_MAX)
REAL(C_FLOAT) :: q_thr, theta_thr, zwt_thr, lai_thr
INTEGER :: spinup_cycles, spinup_years, spinup_min_cycles, spinup_freeze
REAL(C_DOUBLE) :: spinup_tol_water, spinup_tol_zwt, spinup_tol_plant
INTEGER(C_INT64_T) :: seed
NAMELIST /h9gpu/ input_mode, case_dir, out_dir, nlayers, grow_on, device, &
                 grid, year0, nyears, seed, pgf_dir, nc_out, gnx, gny, gnland, &
                 cell_order, ordered_decades, daily, monthly, evap, days, &
                 daystats, q_thr, theta_thr, zwt_thr, lai_thr, &
                 dayquant, quant_series, quant_p, quant_pool, &
                 spinup_cycles, spinup_years, spinup_min_cycles, spinup_freeze, &
                 spinup_tol_water, spinup_tol_zwt, spinup_tol_plant
CHARACTER (LEN = 600, KIND = C_CHAR), TARGET :: pgf_file (7)
TYPE(C_PTR) :: pgf_ptr (7)
CHARACTER (LEN = *), PARAMETER :: pgf_var (7) = &
  (/ 'tas ', 'rlds', 'rsds', 'huss', 'ps  ', 'pr  ', 'rhs ' /)   ! READ_PGF.f90 order
REAL(C_FLOAT) :: zc (H9G_LMAX)
CHARACTER (LEN = 4) :: ydate, ydate2

! --- case.nml of the harness (oracle/ref/h9ref_main.f90) -------------------
INTEGER :: ncell, state_override, ntrace, trace_cells (64), lclim_mode
NAMELIST /h9case/ ncell, NISURF, year0, nyears, grow_on, state_override, &
                  ntrace, trace_cells, lclim_mode, cell_order

TYPE(h9g_config) :: cfg
TYPE(C_PTR) :: ctx
INTEGER(C_INT) :: rc
INTEGER :: L, ndays, iyr, jyear, nt, d0, u, i, nslot, nland, nx, ny
INTEGER :: dsyr, deyr, ndec, k
INTEGER(C_INT32_T), ALLOCATABLE :: slots (:), passes (:)
LOGICAL :: have_driver, have_nml
CHARACTER (LEN = 512) :: arg
REAL(C_FLOAT), ALLOCATABLE :: theta_s (:,:), hksat (:,:), bsw (:,:), psi_s (:,:)
REAL(C_FLOAT), ALLOCATABLE :: Fmax (:), forcing (:,:,:), state (:), annual (:,:), annual_dec (:,:,:)
INTEGER(C_INT64_T), ALLOCATABLE :: gid (:)
REAL(C_FLOAT), ALLOCATABLE :: lat (:)
REAL(C_DOUBLE) :: diag (H9G_NDIAG)
TYPE(h9g_error) :: err
INTEGER :: time_BOY (2300-1860+1)
! --- daily diagnostics (h9g_set_daily): the current decade's lines ---------
INTEGER(C_INT32_T), ALLOCATABLE :: dcells (:)
REAL(C_FLOAT), ALLOCATABLE :: dbuf (:,:,:)
INTEGER, ALLOCATABLE :: dyear (:)
INTEGER :: dfill, dnyr, udaily, ucsv, lon_s_w, lat_s_w, nwin, ix, iy
REAL :: a_lon, b_lon, a_lat, b_lat, lon1, lat1
! --- monthly output (h9g_set_monthly): a year's snapshots and its grid ------
REAL(C_FLOAT), ALLOCATABLE :: mon (:,:,:)
! --- day records (h9g_set_days): a year's records, on the monthly output's grid
REAL(C_FLOAT), ALLOCATABLE :: drec (:,:,:)
INTEGER(C_INT64_T), ALLOCATABLE :: mgid (:)
INTEGER :: mnx, mny
! --- day statistics (h9g_get_daystats): a year's 17 rows; rec_days: day
! recording is on (days or daystats) -----------------------------------------
TYPE(h9g_daystat_opts) :: dopts
REAL(C_DOUBLE), ALLOCATABLE :: dstat (:,:)
INTEGER :: rec_days
! --- day quantiles (h9g_get_dayquant): one result's 1 + 2 nq rows -------------
TYPE(h9g_dayquant_opts) :: qopts
REAL(C_DOUBLE), ALLOCATABLE :: dquant (:,:)
! --- spin-up (h9g_spinup) ---------------------------------------------------
TYPE(h9g_spinup_opts) :: sopts
INTEGER(C_INT32_T) :: scycles
INTEGER(C_INT32_T), ALLOCATABLE :: sslots (:), scell (:)
REAL(C_DOUBLE), ALLOCATABLE :: shist (:,:)

!----------------------------------------------------------------------!
! Defaults, then driver.txt and h9gpu.nml.
!----------------------------------------------------------------------!
input_mode = 'synth'; case_dir = ''; out_dir = '.'; pgf_dir = '.'
nlayers = 8; grow_on = 1; device = 0; grid = 1; year0 = 0; nyears = 0
nc_out = 1; gnx = 0; gny = 0; gnland = 0; cell_order = 1; ordered_decades = 0
monthly = 0; evap = 0; days = 0
daystats = 0; q_thr = 1.0; theta_thr = 0.2; zwt_thr = 1000.0; lai_thr = 1.0
dayquant = 0; quant_series = 0; quant_p = -1.0D0; quant_pool = 0
spinup_cycles = 0; spinup_years = 1; spinup_min_cycles = 1; spinup_freeze = 1
spinup_tol_water = HUGE (1.0D0); spinup_tol_zwt = HUGE (1.0D0); spinup_tol_plant = HUGE (1.0D0)
daily = 0; INTERACTIVE = .FALSE.; lon_w = 0.0; lat_w = 0.0; lon_c_w = 1.0; lat_c_w = 1.0
PATH_output = '.'
seed = 20161123_C_INT64_T
NISURF = 48; iDEC_start = 1; iDEC_end = 1
zi = 0.0
zi (0:9) = (/ 0.0, 45.0, 91.0, 166.0, 289.0, 493.0, 829.0, 1383.0, 2296.0, 5000.0 /)

arg = 'driver.txt'
IF (COMMAND_ARGUMENT_COUNT () >= 1) CALL GET_COMMAND_ARGUMENT (1, arg)
INQUIRE (FILE = TRIM (arg), EXIST = have_driver)
IF (have_driver) CALL read_driver (TRIM (arg))
arg = 'h9gpu.nml'
IF (COMMAND_ARGUMENT_COUNT () >= 2) CALL GET_COMMAND_ARGUMENT (2, arg)
INQUIRE (FILE = TRIM (arg), EXIST = have_nml)
IF (have_nml) THEN
  OPEN (NEWUNIT = u, FILE = TRIM (arg), STATUS = 'OLD')
  READ (u, NML = h9gpu)
  CLOSE (u)
END IF

!----------------------------------------------------------------------!
! Calendar (INIT.f90:844-859).
!----------------------------------------------------------------------!
time_BOY (1) = 1
DO jyear = 1861, 2300
  IF (MOD (jyear-1,4) .NE. 0) THEN
    time_BOY (jyear-1859) = time_BOY (jyear-1859-1) + 365
  ELSE IF (MOD (jyear-1, 100) .NE. 0) THEN
    time_BOY (jyear-1859) = time_BOY (jyear-1859-1) + 366
  ELSE IF (MOD (jyear-1, 400) .NE. 0) THEN
    time_BOY (jyear-1859) = time_BOY (jyear-1859-1) + 365
  ELSE
    time_BOY (jyear-1859) = time_BOY (jyear-1859-1) + 366
  END IF
END DO

!----------------------------------------------------------------------!
! Inputs.
!----------------------------------------------------------------------!
state_override = 0
IF (TRIM (input_mode) == 'case') THEN
  ncell = 0; ntrace = 0; trace_cells = 0; lclim_mode = 0
  OPEN (NEWUNIT = u, FILE = TRIM (case_dir)//'/case.nml', STATUS = 'OLD')
  READ (u, NML = h9case)
  CLOSE (u)
  IF (lclim_mode /= 0) STOP 'h9_host: LCLIM cases run through h9g_run_site (hybrid9_amd.site)'

  nlayers = 8
  L = nlayers
  OPEN (NEWUNIT = u, FILE = TRIM (case_dir)//'/zi.f32', ACCESS = 'STREAM', &
        FORM = 'UNFORMATTED', STATUS = 'OLD')
  READ (u) zi (0:L+1)
  CLOSE (u)
  ALLOCATE (theta_s (L,ncell), hksat (L,ncell), bsw (L,ncell), psi_s (L,ncell))
  ALLOCATE (Fmax (ncell))
  OPEN (NEWUNIT = u, FILE = TRIM (case_dir)//'/params.f32', ACCESS = 'STREAM', &
        FORM = 'UNFORMATTED', STATUS = 'OLD')
  READ (u) theta_s, hksat, bsw, psi_s, Fmax
  CLOSE (u)
  ndays = time_BOY (year0+nyears-1859) - time_BOY (year0-1859)
  ALLOCATE (forcing (ncell, ndays, 7))
  OPEN (NEWUNIT = u, FILE = TRIM (case_dir)//'/forcing.f32', ACCESS = 'STREAM', &
        FORM = 'UNFORMATTED', STATUS = 'OLD')
  READ (u) forcing
  CLOSE (u)
ELSE
  ! synthetic land grid (SURVEY.md §8d): 0.5 deg = 67,420 cells, 0.25 deg
  ! = 270,000 cells with 10 layers
  IF (grid == 1) THEN
    nx = 720; ny = 360; nland = 67420
  ELSE
    nx = 1440; ny = 720; nland = 270000
  END IF
  IF (gnx > 0) nx = gnx
  IF (gny > 0) ny = gny
  IF (gnland > 0) nland = gnland
  ncell = nland
  L = nlayers
  IF (L == 10 .AND. grid == 1 .AND. gnx == 0) STOP 'h9_host: L=10 uses the 0.25 deg grid'
  IF (L == 10) zi (0:11) = (/ 0.0, 18.0, 45.0, 91.0, 166.0, 289.0, 493.0, &
                              829.0, 1383.0, 2296.0, 3500.0, 5000.0 /)
  ALLOCATE (gid (ncell), lat (ncell))
  rc = h9g_land_cells (nx, ny, nland, seed, gid, lat)
  IF (rc /= 0) STOP 'h9_host: h9g_land_cells failed'
  IF (INTERACTIVE) THEN
    ! the focus window (INIT.f90:220-236): the reference's linear maps from
    ! degrees to 1-based indices, its +-179.75 / +-89.75 cell centres written
    ! for any grid; then lon_c = lon_c_w, lat_c = lat_c_w, lon_s = lon_s_w,
    ! lat_s = lat_s_w (:280-283, :462-466) cut the land list to the window
    lon1 = 180.0 - 180.0 / FLOAT (nx)
    lat1 = 90.0 - 90.0 / FLOAT (ny)
    b_lon = (FLOAT (nx) - 1.0) / (lon1 - (-lon1))
    a_lon = 1.0 - b_lon * (-lon1)
    b_lat = (FLOAT (ny) - 1.0) / (-lat1 - lat1)
    a_lat = FLOAT (ny) - b_lat * (-lat1)
    lon_s_w = NINT (a_lon + b_lon * lon_w)
    lat_s_w = NINT (a_lat + b_lat * lat_w)
    WRITE (*,*) 'Details of focus point', lon_w, lat_w, lon_s_w, lat_s_w
    nwin = 0
    DO i = 1, ncell
      ix = INT (MOD (gid (i), INT (nx, C_INT64_T))) + 1
      iy = INT (gid (i) / INT (nx, C_INT64_T)) + 1
      IF (ix >= lon_s_w .AND. ix < lon_s_w + NINT (lon_c_w) .AND. &
          iy >= lat_s_w .AND. iy < lat_s_w + NINT (lat_c_w)) THEN
        nwin = nwin + 1
        gid (nwin) = gid (i)
        lat (nwin) = lat (i)
      END IF
    END DO
    IF (nwin == 0) STOP 'h9_host: INTERACTIVE: the focus window holds no land cell'
    ncell = nwin
    gid = gid (1:ncell)
    lat = lat (1:ncell)
    daily = 1
  END IF
  IF (year0 == 0) year0 = (iDEC_start - 1) * 10 + 1901        ! HYBRID9.f90:103
  IF (nyears == 0) THEN                                        ! HYBRID9.f90:109-113
    eyr = (iDEC_end - 1) * 10 + 1901 + MERGE (9, 1, iDEC_end < 12)
    nyears = eyr - year0 + 1
  END IF
END IF

! layer centre depths for the output (INIT.f90:252-263, zc_o)
DO i = 1, L
  zc (i) = zi (i) - (zi (i) - zi (i-1)) / 2.0
END DO

!----------------------------------------------------------------------!
! GPU context.
!----------------------------------------------------------------------!
nslot = 2                                  ! isolated cells: double-buffered years
IF (cell_order /= 0) THEN                  ! the reference's order: every year of a call resident
  nslot = nyears
  IF (daily /= 0) ordered_decades = 1      ! recorded runs: one h9g_run_decade_ordered per decade
  IF (ordered_decades > 0) nslot = MIN (nyears, 10 * ordered_decades)
END IF
IF (spinup_cycles > 0) THEN                ! the spin-up period resident too
  IF (spinup_years < 1 .OR. spinup_years > nyears) STOP 'h9_host: spinup_years must be in 1 .. nyears'
  nslot = MAX (nslot, spinup_years)
END IF
cfg%ncell = ncell
cfg%nlayers = L
cfg%nisurf = NISURF
cfg%grow_on = grow_on
cfg%max_days = 366
cfg%nslots = nslot
cfg%zi = zi
IF (h9g_abi_version () /= 1) STOP 'h9_host: libh9g ABI mismatch'
IF (h9g_device_count () < 1) STOP 'h9_host: no GPU visible'
ctx = h9g_create (cfg, device)
IF (.NOT. C_ASSOCIATED (ctx)) STOP 'h9_host: h9g_create failed'

IF (TRIM (input_mode) == 'case') THEN
  CALL chk (h9g_set_params (ctx, theta_s, hksat, bsw, psi_s, Fmax))
  IF (state_override /= 0) THEN
    ALLOCATE (state (h9g_state_size (L) * ncell))
    OPEN (NEWUNIT = u, FILE = TRIM (case_dir)//'/state0.f32', ACCESS = 'STREAM', &
          FORM = 'UNFORMATTED', STATUS = 'OLD')
    READ (u) state
    CLOSE (u)
    CALL chk (h9g_set_state (ctx, state))
    DEALLOCATE (state)
  ELSE
    CALL chk (h9g_init_state (ctx))                ! INIT.f90:707-811
  END IF
ELSE
  CALL chk (h9g_set_cells (ctx, gid, lat))
  CALL chk (h9g_synth_params (ctx, seed))
  CALL chk (h9g_init_state (ctx))
END IF

!----------------------------------------------------------------------!
! Spin-up: the run's first spinup_years years repeated until the cells
! settle (h9g_spinup); the run proper then starts from that state.
!----------------------------------------------------------------------!
IF (spinup_cycles > 0) THEN
  ALLOCATE (sslots (spinup_years), scell (ncell), shist (H9G_NSPIN, spinup_cycles))
  d0 = 1
  DO k = 1, spinup_years
    sslots (k) = k - 1
    CALL stage (k - 1, year0 + k - 1, d0)
    d0 = d0 + time_BOY (year0+k-1859) - time_BOY (year0+k-1-1859)
  END DO
  sopts%max_cycles = spinup_cycles
  sopts%min_cycles = spinup_min_cycles
  sopts%freeze = spinup_freeze
  sopts%reserved = 0
  sopts%tol_water = spinup_tol_water
  sopts%tol_zwt = spinup_tol_zwt
  sopts%tol_plant = spinup_tol_plant
  IF (evap /= 0) CALL chk (h9g_set_evap (ctx, 1))
  rc = h9g_spinup (ctx, sslots, year0, spinup_years, sopts, scycles, scell, shist)
  IF (rc < 0) CALL h9g_check_stop (ctx, rc)
  OPEN (NEWUNIT = u, FILE = TRIM (out_dir)//'/spinup.txt', STATUS = 'REPLACE')
  DO k = 1, scycles
    WRITE (u,'(I5,3I10,3ES24.16)') k, NINT (shist (1:3, k)), shist (4:6, k)
  END DO
  CLOSE (u)
  OPEN (NEWUNIT = u, FILE = TRIM (out_dir)//'/spinup_cycle.i32', ACCESS = 'STREAM', &
        FORM = 'UNFORMATTED', STATUS = 'REPLACE')
  WRITE (u) scell
  CLOSE (u)
  WRITE (*,'(A,I5,A,I8,A,I8,A)') ' spin-up:', scycles, ' cycles,', COUNT (scell > 0), ' cells settled,', &
        COUNT (scell == 0), ' still active'
  CALL h9g_check_stop (ctx, rc)
END IF

!----------------------------------------------------------------------!
! Year loop: the GPU replaces HYBRID9.f90:120-295.  Forcing for year y+1
! is pushed (async) into the other slot while year y runs.
!----------------------------------------------------------------------!
ALLOCATE (annual (ncell, 12 + L))
OPEN (NEWUNIT = u, FILE = TRIM (out_dir)//'/annual.f32', ACCESS = 'STREAM', &
      FORM = 'UNFORMATTED', STATUS = 'REPLACE')
IF (daily /= 0) THEN
  ALLOCATE (dcells (ncell), dbuf (ncell, H9G_NDAILY, 366 * MIN (nyears, 10)), dyear (10))
  DO i = 1, ncell
    dcells (i) = i - 1
  END DO
  CALL chk (h9g_set_daily (ctx, ncell, dcells))
  dfill = 0; dnyr = 0
  OPEN (NEWUNIT = udaily, FILE = TRIM (out_dir)//'/daily.f32', ACCESS = 'STREAM', &
        FORM = 'UNFORMATTED', STATUS = 'REPLACE')
  IF (INTERACTIVE) THEN                      ! INIT.f90:887-890
    CALL EXECUTE_COMMAND_LINE ('mkdir -p LCLIM')
    OPEN (NEWUNIT = ucsv, FILE = 'LCLIM/daily_diag.csv', STATUS = 'UNKNOWN')
    WRITE (ucsv,'(A200)') 'jyear,  DOY,  et,  et_g,  theta_1,  theta_2,  &
                  &theta_3,  theta_4,&
                  &  theta_ma_1,  lai,  lai_litter, w_i, fT'
  END IF
END IF
rec_days = 0
IF (days /= 0 .OR. daystats /= 0 .OR. dayquant /= 0) rec_days = 1
IF (rec_days /= 0) evap = 1
IF (evap /= 0) CALL chk (h9g_set_evap (ctx, 1))
IF (monthly /= 0) THEN
  CALL chk (h9g_set_monthly (ctx, 1))
  ALLOCATE (mon (ncell, 12 + L, H9G_NMONTHS))
END IF
IF (rec_days /= 0) CALL chk (h9g_set_days (ctx, 1))
IF (days /= 0) ALLOCATE (drec (ncell, H9G_NDAYREC, 366))
IF (daystats /= 0) THEN
  dopts%q_thr = q_thr; dopts%theta_thr = theta_thr; dopts%zwt_thr = zwt_thr; dopts%lai_thr = lai_thr
  dopts%reserved = 0
  ALLOCATE (dstat (ncell, H9G_NDAYSTAT))
END IF
IF (dayquant /= 0) THEN
  IF (quant_pool /= 0 .AND. cell_order == 0) THEN
    WRITE (*,*) 'h9_host: quant_pool = 1 needs cell_order = 1: an isolated run retains one year'
    STOP 1
  END IF
  IF (ALL (quant_p < 0.0D0)) quant_p (1:3) = (/ 0.05D0, 0.5D0, 0.95D0 /)
  qopts%series = quant_series; qopts%nq = 0; qopts%pooled = quant_pool; qopts%reserved = 0
  qopts%p = 0.0D0
  DO i = 1, H9G_NQUANT_MAX                   ! the entries that were set, in their order
    IF (quant_p (i) >= 0.0D0) THEN
      qopts%nq = qopts%nq + 1
      qopts%p (qopts%nq) = quant_p (i)
    END IF
  END DO
  ALLOCATE (dquant (ncell, 1 + 2 * qopts%nq))
END IF
IF (monthly /= 0 .OR. rec_days /= 0) THEN
  ALLOCATE (mgid (ncell))
  IF (TRIM (input_mode) == 'case') THEN
    mnx = ncell; mny = 1
    DO i = 1, ncell
      mgid (i) = i - 1
    END DO
  ELSE
    mnx = nx; mny = ny
    mgid = gid (1:ncell)
  END IF
END IF
d0 = 1
IF (cell_order /= 0) THEN
  ! HYBRID9.f90:93-130: decade by decade (1901-1910, 1911-1920, ...), cut to
  ! [year0, year0 + nyears); a call's years staged into their slots, then
  ! the cells run in the reference's order, the decades overlapping
  ALLOCATE (annual_dec (ncell, 12 + L, nslot), slots (nslot), passes (nslot / 10 + 2))
  dsyr = year0
  DO WHILE (dsyr < year0 + nyears)
    ! the call's last year: ordered_decades whole decades on from dsyr's
    ! (FLOOR, not integer division, which truncates toward zero: before 1901
    ! the decades are 1891-1900, 1881-1890, ...)
    deyr = year0 + nyears - 1
    IF (ordered_decades > 0) &
      deyr = MIN (deyr, 1901 + 10 * (FLOOR (REAL (dsyr - 1901) / 10.0) + ordered_decades) - 1)
    ndec = deyr - dsyr + 1                   ! years of the call
    DO k = 1, ndec
      slots (k) = k - 1
      CALL stage (k - 1, dsyr + k - 1, d0)
      d0 = d0 + time_BOY (dsyr+k-1859) - time_BOY (dsyr+k-1-1859)
    END DO
    IF (daily /= 0) THEN                     ! (one reference decade per call)
      rc = h9g_run_decade_ordered (ctx, slots, dsyr, ndec, annual_dec, passes (1))
    ELSE
      rc = h9g_run_ordered (ctx, slots, dsyr, ndec, annual_dec, passes)
    END IF
    IF (rc < 0) CALL h9g_check_stop (ctx, rc)
    IF (daily /= 0) THEN
      DO k = 1, ndec
        CALL daily_year (k - 1, dsyr + k - 1)
      END DO
      CALL daily_flush ()
    END IF
    iyr = ndec
    IF (rc > 0) THEN                         ! a STOP: the reference ends in its decade,
      CALL chk (h9g_last_error (ctx, err))   ! after writing the decades before it
      iyr = 1901 + 10 * FLOOR (REAL (err%year - 1901) / 10.0) - dsyr
    END IF
    DO k = 1, iyr
      annual = annual_dec (:, :, k)
      CALL year_out (dsyr + k - 1)
      IF (monthly /= 0) CALL month_out (k - 1, dsyr + k - 1)
      IF (days /= 0) CALL days_out (k - 1, dsyr + k - 1)
      IF (daystats /= 0) CALL stats_out (k - 1, dsyr + k - 1)
      IF (dayquant /= 0 .AND. quant_pool == 0) CALL quant_out (k - 1, 1, dsyr + k - 1)
    END DO
    IF (dayquant /= 0 .AND. quant_pool /= 0 .AND. iyr == ndec) CALL quant_out (0, ndec, dsyr)
    CALL h9g_check_stop (ctx, rc)
    WRITE (*,'(A,I5,A,I5,A,12I3)') ' years', dsyr, ' -', deyr, ' in cell order: passes per decade', &
          passes (1:FLOOR (REAL (deyr - 1901) / 10.0) - FLOOR (REAL (dsyr - 1901) / 10.0) + 1)
    dsyr = deyr + 1
  END DO
ELSE
CALL stage (0, year0, d0)
DO iyr = 1, nyears
  jyear = year0 + iyr - 1
  nt = time_BOY (jyear+1-1859) - time_BOY (jyear-1859)
  CALL chk (h9g_run_year (ctx, MOD (iyr-1, nslot), jyear))
  IF (iyr < nyears) CALL stage (MOD (iyr, nslot), jyear + 1, d0 + nt)
  rc = h9g_sync (ctx)
  CALL h9g_check_stop (ctx, rc)
  CALL chk (h9g_get_annual (ctx, annual))
  CALL year_out (jyear)
  IF (monthly /= 0) CALL month_out (0, jyear)
  IF (days /= 0) CALL days_out (0, jyear)
  IF (daystats /= 0) CALL stats_out (0, jyear)
  IF (dayquant /= 0) CALL quant_out (0, 1, jyear)
  IF (daily /= 0) THEN                       ! flushed at the end of each reference decade
    CALL daily_year (0, jyear)
    IF (MODULO (jyear - 1900, 10) == 0 .OR. iyr == nyears) CALL daily_flush ()
  END IF
  d0 = d0 + nt
END DO
END IF
CLOSE (u)
IF (daily /= 0) THEN
  CLOSE (udaily)
  IF (INTERACTIVE) CLOSE (ucsv)
END IF
ALLOCATE (state (h9g_state_size (L) * ncell))
CALL chk (h9g_get_state (ctx, state))
OPEN (NEWUNIT = u, FILE = TRIM (out_dir)//'/state_end.f32', ACCESS = 'STREAM', &
      FORM = 'UNFORMATTED', STATUS = 'REPLACE')
WRITE (u) state
CLOSE (u)
CALL h9g_destroy (ctx)
WRITE (*,*) 'H9_HOST completed successfully'

CONTAINS

  ! One year's annual means to annual.f32 and axyYYYY.nc, and its line.
  SUBROUTINE year_out (y)
    INTEGER, INTENT(IN) :: y
    WRITE (u) annual
    IF (nc_out /= 0 .AND. TRIM (input_mode) /= 'case') THEN     ! HYBRID9.f90:503-513
      WRITE (ydate,'(I4)') y
      CALL chk (h9g_write_axy_nc (TRIM (PATH_output)//'/axy'//ydate//'.nc'//C_NULL_CHAR, nx, ny, L, &
                                  zc, ncell, gid, annual))
    END IF
    CALL chk (h9g_get_diagnostics (ctx, diag, C_NULL_PTR))    ! (in cell order: the decade's last year)
    WRITE (*,'(A,I5,A,I8,A,ES12.5,A,ES12.5,A,F9.1,A)') ' year', y, ' cells', NINT (diag (1)), &
          ' mean runoff', diag (2) / MAX (diag (1), 1.0D0), ' mm/s  mean soil water', &
          diag (3) / MAX (diag (1), 1.0D0), ' mm  (', h9g_last_kernel_ms (ctx), ' ms)'
  END SUBROUTINE year_out

  ! The month-end snapshots of year k (0-based) of the last run, calendar
  ! year y, as monthly means to <out_dir>/mxyYYYY.nc.
  SUBROUTINE month_out (k, y)
    INTEGER, INTENT(IN) :: k, y
    CALL chk (h9g_get_monthly (ctx, k, mon))
    WRITE (ydate,'(I4)') y
    IF (evap /= 0) THEN
      CALL chk (h9g_write_mxy_nc_evap (TRIM (out_dir)//'/mxy'//ydate//'.nc'//C_NULL_CHAR, mnx, mny, L, zc, &
                                       ncell, mgid, y, NISURF, mon))
    ELSE
      CALL chk (h9g_write_mxy_nc (TRIM (out_dir)//'/mxy'//ydate//'.nc'//C_NULL_CHAR, mnx, mny, L, zc, ncell, &
                                  mgid, y, NISURF, mon))
    END IF
  END SUBROUTINE month_out

  ! The day records of year k (0-based) of the last run, calendar year y, to
  ! <out_dir>/dxyYYYY.nc.
  SUBROUTINE days_out (k, y)
    INTEGER, INTENT(IN) :: k, y
    INTEGER :: n
    n = time_BOY (y+1-1859) - time_BOY (y-1859)
    CALL chk (h9g_get_days (ctx, k, drec))
    WRITE (ydate,'(I4)') y
    CALL chk (h9g_write_dxy_nc (TRIM (out_dir)//'/dxy'//ydate//'.nc'//C_NULL_CHAR, mnx, mny, L, zc, ncell, &
                                mgid, y, n, drec))
  END SUBROUTINE days_out

  ! The day statistics of year k (0-based) of the last run, calendar year y,
  ! to <out_dir>/sxyYYYY.nc.
  SUBROUTINE stats_out (k, y)
    INTEGER, INTENT(IN) :: k, y
    CALL chk (h9g_get_daystats (ctx, k, 1, dopts, dstat))
    WRITE (ydate,'(I4)') y
    CALL chk (h9g_write_sxy_nc (TRIM (out_dir)//'/sxy'//ydate//'.nc'//C_NULL_CHAR, mnx, mny, ncell, mgid, y, &
                                dopts, dstat))
  END SUBROUTINE stats_out

  ! The day quantiles of years k .. k+nk-1 (0-based) of the last run, the
  ! first of them calendar year y: one year to <out_dir>/qxyYYYY.nc, a pooled
  ! span to <out_dir>/qxyYYYY_YYYY.nc.
  SUBROUTINE quant_out (k, nk, y)
    INTEGER, INTENT(IN) :: k, nk, y
    CALL chk (h9g_get_dayquant (ctx, k, nk, qopts, dquant))
    WRITE (ydate,'(I4)') y
    WRITE (ydate2,'(I4)') y + nk - 1
    IF (qopts%pooled /= 0) THEN
      CALL chk (h9g_write_qxy_nc (TRIM (out_dir)//'/qxy'//ydate//'_'//ydate2//'.nc'//C_NULL_CHAR, mnx, mny, ncell, &
                                  mgid, y, y + nk - 1, qopts, dquant))
    ELSE
      CALL chk (h9g_write_qxy_nc (TRIM (out_dir)//'/qxy'//ydate//'.nc'//C_NULL_CHAR, mnx, mny, ncell, mgid, y, y, &
                                  qopts, dquant))
    END IF
  END SUBROUTINE quant_out

  ! The daily lines of year k (0-based) of the last run, calendar year y,
  ! appended to the current decade's.
  SUBROUTINE daily_year (k, y)
    INTEGER, INTENT(IN) :: k, y
    INTEGER :: n
    n = time_BOY (y+1-1859) - time_BOY (y-1859)
    CALL chk (h9g_get_daily (ctx, k, dbuf (:, :, dfill+1:dfill+n)))
    dnyr = dnyr + 1
    dyear (dnyr) = y
    dfill = dfill + n
  END SUBROUTINE daily_year

  ! The decade's lines to daily.f32 (cell fastest, 11, days) and, in the
  ! reference's order (cell, year, day; HYBRID9.f90:120-229), to
  ! LCLIM/daily_diag.csv.  A cell's lines from its STOP on are NaN: the
  ! reference ends before writing them.
  SUBROUTINE daily_flush ()
    INTEGER :: c, j, d, doy, n, i
    IF (dfill == 0) RETURN
    WRITE (udaily) dbuf (:, :, 1:dfill)
    IF (INTERACTIVE) THEN
      DO c = 1, ncell
        d = 0
        DO j = 1, dnyr
          n = time_BOY (dyear (j)+1-1859) - time_BOY (dyear (j)-1859)
          DO doy = 1, n
            d = d + 1
            IF (dbuf (c, 1, d) /= dbuf (c, 1, d)) CYCLE
            WRITE (ucsv,'(2(I5,A1),10(F10.4,A1),F10.4)') dyear (j), ',', doy, ',', &
                  (dbuf (c, i, d), ',', i = 1, 10), dbuf (c, 11, d)
          END DO
        END DO
      END DO
    END IF
    dfill = 0; dnyr = 0
  END SUBROUTINE daily_flush

  SUBROUTINE chk (r)
    INTEGER(C_INT), INTENT(IN) :: r
    IF (r /= 0) CALL h9g_check_stop (ctx, r)
  END SUBROUTINE chk

  ! Forcing of calendar year y into slot s (READ_PGF.f90 equivalent).
  SUBROUTINE stage (s, y, dfirst)
    INTEGER, INTENT(IN) :: s, y, dfirst
    INTEGER :: n
    INTEGER :: idec, dsyr, deyr, k
    CHARACTER (LEN = 9) :: decade
    n = time_BOY (y+1-1859) - time_BOY (y-1859)
    IF (TRIM (input_mode) == 'case') THEN
      CALL chk (h9g_push_forcing (ctx, s, n, forcing (:, dfirst:dfirst+n-1, :), 0))
    ELSE IF (TRIM (input_mode) == 'pgf') THEN
      ! decade files of READ_PGF.f90:22-106; day index within the file
      idec = (y - 1901) / 10 + 1
      dsyr = (idec - 1) * 10 + 1901
      deyr = MERGE (dsyr + 9, dsyr + 1, idec < 12)
      WRITE (decade,'(I4,A,I4)') dsyr, '_', deyr
      DO k = 1, 7
        pgf_file (k) = TRIM (pgf_dir)//'/'//TRIM (pgf_var (k))//'_pgfv2.1_'//decade//'.nc4'//C_NULL_CHAR
        pgf_ptr (k) = C_LOC (pgf_file (k))
      END DO
      CALL chk (h9g_nc_forcing_prefetch (ctx, s, pgf_ptr, nx, ny, &
                                         time_BOY (y-1859) - time_BOY (dsyr-1859), n))
    ELSE
      CALL chk (h9g_synth_forcing (ctx, s, seed, time_BOY (y-1859) - time_BOY (1901-1859), n))
    END IF
  END SUBROUTINE stage

  ! INIT.f90:181-204 list-directed read of driver.txt.
  SUBROUTINE read_driver (fname)
    CHARACTER (LEN = *), INTENT(IN) :: fname
    INTEGER :: v, k
    OPEN (NEWUNIT = v, FILE = fname, STATUS = 'OLD')
    READ (v,*) PATH_output
    READ (v,*) NISURF
    READ (v,*) PGF
    READ (v,*) iDEC_start
    READ (v,*) iDEC_end
    READ (v,*) INTERACTIVE
    READ (v,*) LCLIM
    READ (v,*) LCLIM_filename
    READ (v,*) LSOIL_filename
    READ (v,*) syr
    READ (v,*) eyr
    READ (v,*) NYR_SPIN_UP
    READ (v,*) lon_w
    READ (v,*) lat_w
    READ (v,*) lon_c_w
    READ (v,*) lat_c_w
    DO k = 0, 9
      READ (v,*) zi (k)
    END DO
    CLOSE (v)
    IF (.NOT. PGF) STOP 'h9_host: only the PGF path (HYBRID9.f90:87-337) is supported'
  END SUBROUTINE read_driver

END PROGRAM H9_HOST
!======================================================================!
