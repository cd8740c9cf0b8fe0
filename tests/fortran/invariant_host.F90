! invariant_host.F90 -- a Fortran host with rank-invariant atmosphere sums (test harness, not the
! product).
!
! received_host.F90's frame (local_field held by the reference's flux_calculator_basic, the
! drop-in module's engine) around fcx_define_atmos_terms: ONE process runs a global case and its
! two shards, each through the drop-in module, and completes the shards' shared atmosphere cell
! as a coupled run would -- the boundary slots live in library host memory (fcx_host_malloc, which
! the device reads and writes in place), the "all-reduce" is the host adding the two shards'
! slots, and fcx_atmos_finish adds the terms in link order.  max_terms and left_pos come from the
! table loop of INTEGRATION.md section 3 over the shards' (a0, a1, n0, n1).  The module holds one
! engine at a time, so the shards run twice: once to fill their slots, once more to finish with
! the sum of both.  tests/test_fortran_invariant.py compares the shards' atmosphere fields with
! the global run's, bit for bit.
!
!   invariant_host <global dir> <shard 0 dir> <shard 1 dir>
!
! <dir>/manifest.txt: the records of dropin_host.F90 (N A S M C V R O) and
!   T n_atmos offset file   the exchange -> atmosphere map: file holds the 0-based local atmosphere
!                           cell of every exchange cell (as REAL(8)), then the weights; offset is
!                           the global index of the first local atmosphere cell
!   F s g v file            local_field(s,g)%var(v) is accumulated at the end of the normal phase;
!                           file: the n_atmos sums this host writes
PROGRAM invariant_host
    USE flux_calculator_basic
    USE flux_calculator_calculate
    USE fcx_c_api
    USE, INTRINSIC :: iso_c_binding
    IMPLICIT NONE

    TYPE buf_t
        REAL(wp), POINTER :: p(:) => NULL()
    END TYPE buf_t
    TYPE out_t
        REAL(c_double), POINTER :: p(:) => NULL()
    END TYPE out_t
    TYPE(local_fields_type), TARGET :: local_field(0:MAX_SURFACE_TYPES, 3)
    TYPE(buf_t), ALLOCATABLE :: bufs(:)
    TYPE(out_t) :: aout(32)
    CHARACTER(len=20) :: tables(MAX_BOTTOM_MODELS, MAX_SURFACE_TYPES, 8)
    INTEGER :: grid_size(3), nsurf, init_date, nav, nacc, n_atmos, a_off
    INTEGER :: av(3, 100), acc(3, 32)
    CHARACTER(len=512) :: accpath(32)
    REAL(wp), ALLOCATABLE, TARGET :: corr(:,:)
    INTEGER(c_int32_t), POINTER :: aidx(:) => NULL()
    REAL(c_double), POINTER :: aw(:) => NULL()
    LOGICAL :: lcorr
    CHARACTER(len=1024) :: dirs(0:2)
    ! the shards' table (a0, a1, n0, n1), their slots, and the reduced region
    INTEGER :: every(4, 0:1), left(0:1), right(0:1), left_pos(0:1), max_terms, columns, r, pass
    REAL(c_double), POINTER :: region(:) => NULL()
    REAL(c_double), ALLOCATABLE :: saved(:,:)

    CALL get_command_argument(1, dirs(2))  ! the global case
    CALL get_command_argument(2, dirs(0))
    CALL get_command_argument(3, dirs(1))
    w_unit = 6
    CALL init_varname_idx

    ! ---- every rank's four numbers, "gathered": (a0, a1, n0, n1) of its range
    DO r = 0, 1
        CALL load(TRIM(dirs(r)))
        every(:, r) = (/ a_off, a_off + n_atmos - 1, COUNT(aidx == 0), COUNT(aidx == n_atmos - 1) /)
    ENDDO
    CALL terms_table(every, 2, left_pos, max_terms)
    left = -1
    right = -1
    IF (every(2, 0) == every(1, 1)) THEN  ! the one boundary cuts an atmosphere cell
        right(0) = 0
        left(1) = 0
    ENDIF
    IF (left(1) < 0) ERROR STOP 'invariant_host: the shards share no atmosphere cell'

    ! ---- the global run: one rank, the option off
    CALL load(TRIM(dirs(2)))
    CALL start_engine(-1)
    CALL run_step()
    CALL write_sums(TRIM(dirs(2)))
    CALL fcx_detach()

    ! ---- the shards: pass 1 fills each shard's slots, pass 2 finishes with their sum
    DO pass = 1, 2
        DO r = 0, 1
            CALL load(TRIM(dirs(r)))
            CALL start_engine(r)
            CALL run_step()
            IF (pass == 1) THEN
                IF (.NOT. ALLOCATED(saved)) ALLOCATE (saved(columns, 0:1))
                saved(:, r) = region(1:columns)
            ELSE
                region(1:columns) = saved(:, 0) + saved(:, 1)  ! every term slot: x + 0
                CALL must(fcx_atmos_finish(fcx_engine_handle()), 'fcx_atmos_finish')
                CALL must(fcx_download(fcx_engine_handle(), FCX_PHASE_NORMAL), 'fcx_download')
                CALL must(fcx_synchronize(fcx_engine_handle()), 'fcx_synchronize')
                IF (ANY(region(1:columns) /= 0.0_c_double)) ERROR STOP 'invariant_host: slots not re-zeroed'
                CALL write_sums(TRIM(dirs(r)))
            ENDIF
            CALL fcx_detach()
        ENDDO
    ENDDO
    WRITE (*, '(A,I0,A,I0,A,I0)') 'INVARIANT_HOST OK max_terms ', max_terms, ' left_pos ', left_pos(1), &
        ' columns ', columns

CONTAINS

    ! INTEGRATION.md section 3: left_pos of every rank and K from the ranks' (a0, a1, n0, n1)
    SUBROUTINE terms_table(tab, nranks, lpos, k)
        INTEGER, INTENT(IN)  :: nranks, tab(4, 0:nranks - 1)
        INTEGER, INTENT(OUT) :: lpos(0:nranks - 1), k
        INTEGER :: q, pos, run, prev
        lpos = 0
        k = 1
        run = 0
        prev = -1
        DO q = 0, nranks - 1
            IF (tab(3, q) == 0) CYCLE
            pos = 0
            IF (tab(1, q) == prev) pos = run
            lpos(q) = pos
            IF (pos > 0) k = MAX(k, pos + tab(3, q))
            run = tab(4, q)
            IF (tab(1, q) == tab(2, q)) run = pos + tab(3, q)
            prev = tab(2, q)
        ENDDO
    END SUBROUTINE terms_table

    ! attach the loaded case; rank >= 0: a shard with the option on and its slots
    SUBROUTINE start_engine(rank)
        INTEGER, INTENT(IN) :: rank
        TYPE(c_ptr) :: h, blk
        INTEGER(c_int32_t) :: cols, on
        INTEGER :: i
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
        h = fcx_engine_handle()
        IF (rank >= 0) CALL fcx_define_atmos_terms(max_terms, left_pos(rank))
        CALL must(fcx_set_atmos_map(h, INT(n_atmos, c_int64_t), C_LOC(aidx(1)), C_LOC(aw(1))), 'fcx_set_atmos_map')
        DO i = 1, nacc
            CALL must(fcx_add_atmos_field(h, FCX_PHASE_NORMAL, INT(acc(1, i), c_int), INT(acc(2, i), c_int), &
                                          INT(acc(3, i), c_int), C_LOC(aout(i)%p(1)), FCX_MEM_HOST), 'fcx_add_atmos_field')
        ENDDO
        CALL must(fcx_atmos_invariant(h, on), 'fcx_atmos_invariant')
        IF ((on == 1) .NEQV. (rank >= 0)) ERROR STOP 'invariant_host: fcx_atmos_invariant disagrees'
        CALL must(fcx_atmos_columns(h, cols), 'fcx_atmos_columns')
        IF (rank >= 0) THEN
            IF (cols /= nacc * (1 + max_terms)) ERROR STOP 'invariant_host: fcx_atmos_columns is not fields x (1 + K)'
            columns = cols
            CALL must(fcx_host_malloc(INT(columns, c_size_t) * 8_c_size_t, blk), 'fcx_host_malloc')
            CALL C_F_POINTER(blk, region, [columns])
            region = 0.0_c_double
            CALL must(fcx_set_atmos_shared(h, blk, 1_c_int32_t, cols, INT(left(rank), c_int32_t), &
                                           INT(right(rank), c_int32_t)), 'fcx_set_atmos_shared')
        ELSE
            IF (cols /= nacc) ERROR STOP 'invariant_host: fcx_atmos_columns is not the field count with the option off'
        ENDIF
        CALL fcx_commit_engine()
    END SUBROUTINE start_engine

    SUBROUTINE run_step()
        CALL fcx_run_phase(FCX_PHASE_EARLY)
        CALL fcx_run_phase(FCX_PHASE_NORMAL)
        CALL must(fcx_synchronize(fcx_engine_handle()), 'fcx_synchronize')
    END SUBROUTINE run_step

    SUBROUTINE write_sums(dir)
        CHARACTER(len=*), INTENT(IN) :: dir
        INTEGER :: i
        DO i = 1, nacc
            CALL write_raw(dir//'/'//TRIM(accpath(i)), aout(i)%p)
        ENDDO
    END SUBROUTINE write_sums

    SUBROUTINE must(status, what)
        INTEGER(c_int), INTENT(IN) :: status
        CHARACTER(len=*), INTENT(IN) :: what
        IF (status /= FCX_OK) THEN
            WRITE (*, '(A)') 'invariant_host: '//what//': '//TRIM(fcx_error_message())
            ERROR STOP 3
        ENDIF
    END SUBROUTINE must

    ! the manifest of one case into local_field and the map (what an earlier load left is dropped)
    SUBROUTINE load(dir)
        CHARACTER(len=*), INTENT(IN) :: dir
        INTEGER :: u, ios, nbufs, k, n, s, g, v, alloc, tbl, i
        REAL(8), ALLOCATABLE :: tmp(:)
        CHARACTER(len=1024) :: line, path
        CHARACTER(len=4) :: tag
        CHARACTER(len=20) :: meth
        DO s = 0, MAX_SURFACE_TYPES
            DO g = 1, 3
                CALL nullify_localvars(local_field(s, g))
            ENDDO
        ENDDO
        IF (ALLOCATED(bufs)) DEALLOCATE (bufs)
        IF (ALLOCATED(corr)) DEALLOCATE (corr)
        tables = 'none'
        lcorr = .FALSE.
        init_date = 0
        nav = 0
        nacc = 0
        OPEN (NEWUNIT=u, FILE=dir//'/manifest.txt', STATUS='old', ACTION='read')
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
                CALL read_raw(dir//'/'//TRIM(path), tmp)
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
                CALL read_raw(dir//'/'//TRIM(path), tmp)
                corr = RESHAPE(REAL(tmp, wp), [12, grid_size(1)])
                DEALLOCATE (tmp)
                lcorr = .TRUE.
            CASE ('V')
                nav = nav + 1
                READ (line, *) tag, av(1, nav), av(2, nav), av(3, nav)
            CASE ('R')
                READ (line, *) tag, current_step_time
            CASE ('T')
                READ (line, *) tag, n_atmos, a_off, path
                n = grid_size(1)
                ALLOCATE (aidx(n), aw(n), tmp(2 * n))
                CALL read_raw(dir//'/'//TRIM(path), tmp)
                aidx = NINT(tmp(1:n))
                aw = tmp(n + 1:2 * n)
                DEALLOCATE (tmp)
            CASE ('F')
                nacc = nacc + 1
                READ (line, *) tag, acc(1, nacc), acc(2, nacc), acc(3, nacc), accpath(nacc)
            END SELECT
        ENDDO
        CLOSE (u)
        DO i = 1, nacc
            ALLOCATE (aout(i)%p(MAX(n_atmos, 1)))
            aout(i)%p = -1.0_c_double
        ENDDO
    END SUBROUTINE load

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

END PROGRAM invariant_host

! The host program's MPI finalisation: flux_calculator_basic calls mpi_finalize(1) on a
! configuration error; this single-rank test host has no MPI, so such an error ends the run here.
SUBROUTINE mpi_finalize(ierror)
    INTEGER :: ierror
    WRITE (*, '(A,I0)') 'mpi_finalize called by flux_calculator_basic, code ', ierror
    ERROR STOP 2
END SUBROUTINE mpi_finalize
