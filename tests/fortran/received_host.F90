! received_host.F90 -- a Fortran host that receives its atmosphere fields on the model's grid
! (test harness, not the product).
!
! dropin_host.F90's frame around the receive side of the drop-in module: local_field is held by
! the reference's own flux_calculator_basic, the engine is attached, and -- in mode `declared`
! -- every X record's field is declared with fcx_define_receive_map / fcx_declare_received: the
! host "receives" the model-grid values into a source array, and the exchange-grid array it
! would have received into is overwritten with NaN once the engine is committed.  In mode
! `plain` the P and X records are ignored and the exchange-grid arrays of the manifest (which
! tests/test_fortran_received.py expanded on the host) are used as ever.  Both modes run the
! two fused phases and write the outputs; the test compares them bit for bit.
!
!   received_host <dir> declared|plain
!
! <dir>/manifest.txt: the records of dropin_host.F90 (N A S M C V R O) and
!   P id g n_src n_links file   receive map `id` onto grid g: file holds src(1:n_links),
!                               dst(1:n_links) (1-based, as REAL(8)) and weight(1:n_links)
!   X s g v id phase file       local_field(s,g)%var(v) is received through map id before
!                               phase (1 early, 2 normal); file: its n_src model-grid values
PROGRAM received_host
    USE flux_calculator_basic
    USE flux_calculator_calculate
    USE fcx_c_api, ONLY: FCX_PHASE_EARLY, FCX_PHASE_NORMAL
    USE, INTRINSIC :: iso_c_binding, ONLY: c_int
    USE, INTRINSIC :: ieee_arithmetic, ONLY: ieee_value, ieee_quiet_nan
    IMPLICIT NONE

    TYPE buf_t
        REAL(wp), POINTER :: p(:) => NULL()
    END TYPE buf_t
    TYPE map_t
        INTEGER :: g = 0, n_src = 0, n_links = 0, handle = -1
        INTEGER, ALLOCATABLE :: src(:), dst(:)
        REAL(wp), ALLOCATABLE :: w(:)
    END TYPE map_t
    TYPE(local_fields_type), TARGET :: local_field(0:MAX_SURFACE_TYPES, 3)
    TYPE(buf_t), ALLOCATABLE :: bufs(:)
    TYPE(buf_t) :: sources(200)
    TYPE(map_t) :: maps(8)
    CHARACTER(len=20) :: tables(MAX_BOTTOM_MODELS, MAX_SURFACE_TYPES, 8)
    INTEGER :: grid_size(3), nsurf, nbufs, k, n, s, g, v, alloc, tbl, init_date, ios, u, i, id
    INTEGER :: nav, nout, nrecv
    INTEGER :: av(3, 100), outs(3, 200), recv(5, 200)
    CHARACTER(len=512) :: outpath(200)
    REAL(wp), ALLOCATABLE, TARGET :: corr(:,:)
    REAL(8), ALLOCATABLE :: tmp(:)
    LOGICAL :: lcorr, declared
    CHARACTER(len=1024) :: dir, mode, line, path
    CHARACTER(len=4) :: tag
    CHARACTER(len=20) :: meth

    CALL get_command_argument(1, dir)
    CALL get_command_argument(2, mode)
    declared = TRIM(mode) == 'declared'
    w_unit = 6
    CALL init_varname_idx
    DO s = 0, MAX_SURFACE_TYPES
        DO g = 1, 3
            CALL nullify_localvars(local_field(s, g))
        ENDDO
    ENDDO
    tables = 'none'
    lcorr = .FALSE.
    init_date = 0
    nav = 0
    nout = 0
    nrecv = 0

    OPEN (NEWUNIT=u, FILE=TRIM(dir)//'/manifest.txt', STATUS='old', ACTION='read')
    DO
        READ (u, '(A)', IOSTAT=ios) line
        IF (ios /= 0) EXIT
        READ (line, *) tag
        SELECT CASE (TRIM(tag))
        CASE ('N')
            READ (line, *) tag, nbufs, nsurf, grid_size(1), grid_size(2), grid_size(3)
            ALLOCATE (bufs(nbufs))
        CASE ('A')
            READ (line, *) tag, k, n, path
            ALLOCATE (bufs(k)%p(n), tmp(n))
            CALL read_raw(TRIM(dir)//'/'//TRIM(path), tmp)
            bufs(k)%p = REAL(tmp, wp)
            DEALLOCATE (tmp)
        CASE ('S')
            READ (line, *) tag, s, g, v, k, alloc
            local_field(s, g)%var(v)%field => bufs(k)%p
            local_field(s, g)%var(v)%allocated = alloc == 1
        CASE ('M')
            READ (line, *) tag, tbl, s, meth
            tables(1, s, tbl) = meth
        CASE ('C')
            READ (line, *) tag, init_date, path
            ALLOCATE (corr(12, grid_size(1)), tmp(12 * grid_size(1)))
            CALL read_raw(TRIM(dir)//'/'//TRIM(path), tmp)
            corr = RESHAPE(REAL(tmp, wp), [12, grid_size(1)])
            DEALLOCATE (tmp)
            lcorr = .TRUE.
        CASE ('V')
            nav = nav + 1
            READ (line, *) tag, av(1, nav), av(2, nav), av(3, nav)
        CASE ('R')
            READ (line, *) tag, current_step_time
        CASE ('O')
            nout = nout + 1
            READ (line, *) tag, outs(1, nout), outs(2, nout), outs(3, nout), outpath(nout)
        CASE ('P')
            READ (line, *) tag, id, g, n, k, path
            maps(id)%g = g
            maps(id)%n_src = n
            maps(id)%n_links = k
            ALLOCATE (maps(id)%src(k), maps(id)%dst(k), maps(id)%w(k), tmp(3 * k))
            CALL read_raw(TRIM(dir)//'/'//TRIM(path), tmp)
            maps(id)%src = NINT(tmp(1:k))
            maps(id)%dst = NINT(tmp(k + 1:2 * k))
            maps(id)%w = REAL(tmp(2 * k + 1:3 * k), wp)
            DEALLOCATE (tmp)
        CASE ('X')
            nrecv = nrecv + 1
            READ (line, *) tag, recv(1, nrecv), recv(2, nrecv), recv(3, nrecv), recv(4, nrecv), recv(5, nrecv), path
            n = maps(recv(4, nrecv))%n_src
            ALLOCATE (sources(nrecv)%p(n), tmp(n))
            CALL read_raw(TRIM(dir)//'/'//TRIM(path), tmp)  ! the host's oasis_get on the model's grid
            sources(nrecv)%p = REAL(tmp, wp)
            DEALLOCATE (tmp)
        END SELECT
    ENDDO
    CLOSE (u)

    IF (lcorr) THEN
        CALL fcx_attach(1, nsurf, grid_size, local_field, tables(:,:,1), tables(:,:,2), tables(:,:,3),   &
                        tables(:,:,4), tables(:,:,5), tables(:,:,6), tables(:,:,7), tables(:,:,8),    &
                        lcorr, init_date, corr)
    ELSE
        CALL fcx_attach(1, nsurf, grid_size, local_field, tables(:,:,1), tables(:,:,2), tables(:,:,3),   &
                        tables(:,:,4), tables(:,:,5), tables(:,:,6), tables(:,:,7), tables(:,:,8),    &
                        lcorr, init_date)
    ENDIF
    IF (declared) THEN
        DO id = 1, SIZE(maps)
            IF (maps(id)%g == 0) CYCLE
            CALL fcx_define_receive_map(maps(id)%g, maps(id)%n_src, maps(id)%src, maps(id)%dst, maps(id)%w, &
                                        maps(id)%handle)
        ENDDO
        DO i = 1, nrecv
            IF (recv(5, i) == 1) THEN
                CALL fcx_declare_received(recv(1, i), recv(2, i), recv(3, i), maps(recv(4, i))%handle, &
                                          FCX_PHASE_EARLY, sources(i)%p, local_field)
            ELSE
                CALL fcx_declare_received(recv(1, i), recv(2, i), recv(3, i), maps(recv(4, i))%handle, &
                                          FCX_PHASE_NORMAL, sources(i)%p, local_field)
            ENDIF
        ENDDO
    ENDIF
    DO i = 1, nav
        CALL fcx_register_average(av(1, i) == 1, av(2, i), av(3, i))
    ENDDO
    CALL fcx_commit_engine()
    IF (declared) THEN  ! the released exchange-grid arrays: never read again
        DO i = 1, nrecv
            local_field(recv(1, i), recv(2, i))%var(recv(3, i))%field = ieee_value(1.0_wp, ieee_quiet_nan)
        ENDDO
    ENDIF
    CALL fcx_run_phase(FCX_PHASE_EARLY)
    CALL fcx_run_phase(FCX_PHASE_NORMAL)
    CALL fcx_detach()

    DO i = 1, nout
        s = outs(1, i)
        g = outs(2, i)
        v = outs(3, i)
        CALL write_raw(TRIM(dir)//'/'//TRIM(outpath(i)), REAL(local_field(s, g)%var(v)%field, 8))
    ENDDO
    WRITE (*, '(A)') 'RECEIVED_HOST OK'

CONTAINS

    SUBROUTINE read_raw(fname, x)
        CHARACTER(len=*), INTENT(IN) :: fname
        REAL(8), INTENT(OUT) :: x(:)
        INTEGER :: uu
        OPEN (NEWUNIT=uu, FILE=fname, ACCESS='stream', FORM='unformatted', STATUS='old', ACTION='read')
        READ (uu) x
        CLOSE (uu)
    END SUBROUTINE read_raw

    SUBROUTINE write_raw(fname, x)
        CHARACTER(len=*), INTENT(IN) :: fname
        REAL(8), INTENT(IN) :: x(:)
        INTEGER :: uu
        OPEN (NEWUNIT=uu, FILE=fname, ACCESS='stream', FORM='unformatted', STATUS='replace', ACTION='write')
        WRITE (uu) x
        CLOSE (uu)
    END SUBROUTINE write_raw

END PROGRAM received_host

! The host program's MPI finalisation: flux_calculator_basic calls mpi_finalize(1) on a
! configuration error; this single-rank test host has no MPI, so such an error ends the run here.
SUBROUTINE mpi_finalize(ierror)
    INTEGER :: ierror
    WRITE (*, '(A,I0)') 'mpi_finalize called by flux_calculator_basic, code ', ierror
    ERROR STOP 2
END SUBROUTINE mpi_finalize
