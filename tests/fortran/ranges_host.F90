! ranges_host.F90 -- a Fortran host with the non-finite guard on (test harness, not the product).
!
! received_host.F90's frame (local_field held by the reference's own flux_calculator_basic, the
! manifest of dropin_host.F90) around the two lines a host adds for the guard and its DEBUG
! range lines: the abort routine is registered, fcx_check_finite(3) is called before
! fcx_commit_engine, the two fused phases run, and for every sent field (O record) the host
! prints what fcx_field_range_of answers and writes the downloaded array.  When a phase finds a
! NaN or an Inf the drop-in hands the message to the abort routine, which prints it and ends the
! program with status 3 -- as a coupled host's would call oasis_abort.
!
!   ranges_host <dir>
PROGRAM ranges_host
    USE flux_calculator_basic
    USE flux_calculator_calculate
    USE fcx_c_api, ONLY: FCX_PHASE_EARLY, FCX_PHASE_NORMAL
    USE, INTRINSIC :: iso_c_binding, ONLY: c_funloc, c_char
    IMPLICIT NONE

    INTERFACE
        SUBROUTINE host_abort(msg) BIND(C)
            IMPORT :: c_char
            CHARACTER(kind=c_char), DIMENSION(*), INTENT(IN) :: msg
        END SUBROUTINE host_abort
    END INTERFACE

    TYPE buf_t
        REAL(wp), POINTER :: p(:) => NULL()
    END TYPE buf_t
    TYPE(local_fields_type), TARGET :: local_field(0:MAX_SURFACE_TYPES, 3)
    TYPE(buf_t), ALLOCATABLE :: bufs(:)
    CHARACTER(len=20) :: tables(MAX_BOTTOM_MODELS, MAX_SURFACE_TYPES, 8)
    INTEGER :: grid_size(3), nsurf, nbufs, k, n, s, g, v, alloc, tbl, init_date, ios, u, i
    INTEGER :: nav, nout, n_bad
    INTEGER :: av(3, 100), outs(3, 200)
    CHARACTER(len=512) :: outpath(200)
    REAL(wp), ALLOCATABLE, TARGET :: corr(:,:)
    REAL(8), ALLOCATABLE :: tmp(:)
    REAL(wp) :: vmin, vmax
    LOGICAL :: lcorr
    CHARACTER(len=1024) :: dir, line, path
    CHARACTER(len=4) :: tag
    CHARACTER(len=20) :: meth

    CALL get_command_argument(1, dir)
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
        END SELECT
    ENDDO
    CLOSE (u)

    CALL fcx_register_abort(c_funloc(host_abort))
    IF (lcorr) THEN
        CALL fcx_attach(1, nsurf, grid_size, local_field, tables(:,:,1), tables(:,:,2), tables(:,:,3),   &
                        tables(:,:,4), tables(:,:,5), tables(:,:,6), tables(:,:,7), tables(:,:,8),    &
                        lcorr, init_date, corr)
    ELSE
        CALL fcx_attach(1, nsurf, grid_size, local_field, tables(:,:,1), tables(:,:,2), tables(:,:,3),   &
                        tables(:,:,4), tables(:,:,5), tables(:,:,6), tables(:,:,7), tables(:,:,8),    &
                        lcorr, init_date)
    ENDIF
    DO i = 1, nav
        CALL fcx_register_average(av(1, i) == 1, av(2, i), av(3, i))
    ENDDO
    CALL fcx_check_finite(3)
    CALL fcx_commit_engine()
    CALL fcx_run_phase(FCX_PHASE_EARLY)
    CALL fcx_run_phase(FCX_PHASE_NORMAL)
    DO i = 1, nout  ! the host's DEBUG lines of its sent fields (flux_calculator.F90:1011-1013)
        CALL fcx_field_range_of(outs(1, i), outs(2, i), outs(3, i), vmin, vmax, n_bad)
        WRITE (*, '(A,3(1X,I0),2(1X,ES24.16E3),1X,I0)') 'RANGE', outs(1, i), outs(2, i), outs(3, i), vmin, vmax, n_bad
    ENDDO
    CALL fcx_detach()

    DO i = 1, nout
        s = outs(1, i)
        g = outs(2, i)
        v = outs(3, i)
        CALL write_raw(TRIM(dir)//'/'//TRIM(outpath(i)), REAL(local_field(s, g)%var(v)%field, 8))
    ENDDO
    WRITE (*, '(A)') 'RANGES_HOST OK'

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

END PROGRAM ranges_host

! The coupled host's abort routine (test stand-in for one that calls oasis_abort(comp_id,
! comp_name, msg)): prints the message it was handed and ends the program
SUBROUTINE host_abort(msg) BIND(C)
    USE, INTRINSIC :: iso_c_binding, ONLY: c_char
    USE fcx_c_api, ONLY: fcx_c_string
    CHARACTER(kind=c_char), DIMENSION(*), INTENT(IN) :: msg
    WRITE (*, '(2A)') 'HOST ABORT ROUTINE: ', TRIM(fcx_c_string(msg))
    CALL FLUSH(6)
    STOP 3
END SUBROUTINE host_abort

! The host program's MPI finalisation: flux_calculator_basic calls mpi_finalize(1) on a
! configuration error; this single-rank test host has no MPI, so such an error ends the run here.
SUBROUTINE mpi_finalize(ierror)
    INTEGER :: ierror
    WRITE (*, '(A,I0)') 'mpi_finalize called by flux_calculator_basic, code ', ierror
    ERROR STOP 2
END SUBROUTINE mpi_finalize
