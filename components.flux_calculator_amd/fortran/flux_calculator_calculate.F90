! flux_calculator_calculate.F90 -- drop-in replacement of the reference module
! flux_calculator_calculate (/root/reference/src/flux_calculator_calculate.F90) that runs
! the flux path on an MI355X through libfcx (include/fcx.h).
!
! Same module name, same public subroutines, same arguments:
!   calc_spec_vapor_surface, calc_flux_mass_evap, calc_flux_heat_latent,
!   calc_flux_heat_sensible, calc_flux_momentum_east, calc_flux_momentum_north,
!   calc_flux_radiation_blackbody, distribute_shortwave_radiation_flux,
!   average_across_surface_types
! plus the engine life cycle the host calls once (INTEGRATION.md):
!   fcx_attach              after flux_calculator.F90:761 (all allocations/aliases final)
!   fcx_register_average    for each type-0 output (optional: fused averaging)
!   fcx_declare_constant    for each input the namelist gave a value (val_*_var_*) instead of
!                           a sender (optional: the field is then never transferred)
!   fcx_define_receive_map /  for each input the host receives on its model's grid (optional: the
!   fcx_declare_received    engine expands it to the exchange grid on the device)
!   fcx_define_atmos_terms  once (optional: atmosphere sums that are the same bits for any number
!                           of ranks, FCX_OPT_ATMOS_INVARIANT)
!   fcx_select_outputs      once, with the host's output_field (optional: the computed fluxes no
!                           output_field entry sends are neither downloaded nor, where nothing
!                           else reads them, stored)
!   fcx_commit_engine       validate + device mirrors
!   fcx_run_phase           fused coupling-step phase (replaces :902 and :972-991)
!   fcx_start_phase /       the same phase in two halves: started (inputs taken, launch and
!   fcx_finish_phase        downloads queued), then completed (outputs in local_field), so
!                           the host can do other work -- e.g. an oasis_get -- in between
!   fcx_detach              at finalisation
! The per-call subroutines keep the reference's exact semantics (each uploads what it
! reads, computes on the GPU, downloads what it writes).  Errors are written to w_unit,
! handed to the host's abort routine when one is registered (fcx_register_abort: a routine
! that calls oasis_abort, as the reference does on a failed exchange, flux_calculator.F90:
! 883-887, so the other components do not wait forever in their next exchange) and stop
! the rank.
MODULE flux_calculator_calculate

    USE flux_calculator_basic
    USE fcx_c_api
    USE, INTRINSIC :: iso_c_binding

    IMPLICIT NONE
    PRIVATE

    PUBLIC calc_spec_vapor_surface
    PUBLIC calc_flux_mass_evap
    PUBLIC calc_flux_heat_latent
    PUBLIC calc_flux_heat_sensible
    PUBLIC calc_flux_momentum_east
    PUBLIC calc_flux_momentum_north
    PUBLIC calc_flux_radiation_blackbody
    PUBLIC distribute_shortwave_radiation_flux
    PUBLIC average_across_surface_types
    PUBLIC fcx_attach, fcx_register_average, fcx_commit_engine, fcx_run_phase, fcx_detach
    PUBLIC fcx_register_abort, fcx_start_phase, fcx_finish_phase, fcx_hand_over_field
    PUBLIC fcx_allocate_field, fcx_free_field
    PUBLIC fcx_declare_constant
    PUBLIC fcx_select_outputs
    PUBLIC fcx_define_receive_map, fcx_declare_received
    PUBLIC fcx_check_finite, fcx_field_range_of, fcx_define_atmos_terms, fcx_engine_handle
    PUBLIC fcx_declare_areas, fcx_field_integral_of

    TYPE(c_ptr), SAVE :: engine = c_null_ptr
    ! What fcx_attach bound.  The reference subroutines take the bottom model, the type count,
    ! the method table and grid_size on every call (calc:25-385); the engine takes them once.
    ! Each per-call subroutine checks its own arguments against these and stops with a named
    ! error when they differ or when no engine is attached.
    INTEGER, SAVE :: att_model = -1, att_types = -1, att_grid(3) = -1
    CHARACTER(len=20), SAVE :: att_methods(0:7, MAX_SURFACE_TYPES)

CONTAINS

    ! the host's abort routine: a BIND(C) subroutine with one argument
    ! CHARACTER(kind=c_char), DIMENSION(*) (the NUL-terminated message; fcx_c_string), passed
    ! as c_funloc(routine).  It is called before the rank stops; a routine that calls
    ! oasis_abort(comp_id, comp_name, fcx_c_string(msg)) ends the coupled job.
    SUBROUTINE fcx_register_abort(handler)
        TYPE(c_funptr), INTENT(IN) :: handler
        INTEGER(c_int) :: r
        r = fcx_set_abort_handler(handler)
    END SUBROUTINE fcx_register_abort

    ! Library memory for one local_field array (INTEGRATION.md section 3): the host calls this
    ! where the reference ALLOCATEs the array -- allocate_localvar (basic:288-309) for every
    ! input, do_prepare_calculation (prepare:36-42) for every output -- and frees it with
    ! fcx_free_field after fcx_detach.  fcx_host_malloc hands out consecutive blocks, so in
    ! the reference's order the inputs form one span and the outputs another, and each phase
    ! moves them with one copy per direction (FCX_OPT_LIB_SPANS).
    SUBROUTINE fcx_allocate_field(field, length)
        REAL(wp), POINTER, INTENT(INOUT) :: field(:)
        INTEGER,           INTENT(IN)    :: length
        TYPE(c_ptr) :: blk
        INTEGER(c_size_t) :: bytes
        bytes = INT(MAX(length, 1), c_size_t) * INT(STORAGE_SIZE(1.0_wp) / 8, c_size_t)
        CALL check(fcx_host_malloc(bytes, blk), 'fcx_allocate_field')
        CALL C_F_POINTER(blk, field, [length])
    END SUBROUTINE fcx_allocate_field

    SUBROUTINE fcx_free_field(field)
        REAL(wp), POINTER, INTENT(INOUT) :: field(:)
        IF (.NOT. ASSOCIATED(field)) RETURN
        IF (SIZE(field) > 0) CALL check(fcx_host_free(C_LOC(field(1))), 'fcx_free_field')
        NULLIFY (field)
    END SUBROUTINE fcx_free_field

    ! the end of the rank on an error: message to w_unit, the host's abort routine, stop
    SUBROUTINE stop_run(msg)
        CHARACTER(len=*), INTENT(IN) :: msg
        INTEGER(c_int) :: r
        WRITE (w_unit, '(A)') msg
        CALL FLUSH(w_unit)
        r = fcx_abort(msg // c_null_char)  ! FCX_E_STATE when no routine is registered
        ERROR STOP 1
    END SUBROUTINE stop_run

    SUBROUTINE check(status, where)
        INTEGER(c_int),   INTENT(IN) :: status
        CHARACTER(len=*), INTENT(IN) :: where
        IF (status /= FCX_OK) CALL stop_run('flux engine error in ' // where // ': ' // TRIM(fcx_error_message()))
    END SUBROUTINE check

    SUBROUTINE contract_error(where, msg)
        CHARACTER(len=*), INTENT(IN) :: where, msg
        CALL stop_run('flux engine contract violation in ' // where // ': ' // msg)
    END SUBROUTINE contract_error

    ! the per-call subroutine `where` against the attached engine: an engine exists, and
    ! num_surface_types, grid_size(1:3), my_bottom_model and its method table column are the
    ! ones fcx_attach bound (flux: FCX_* table id; absent for calls that take no table)
    SUBROUTINE require(where, num_surface_types, grid_size, my_bottom_model, flux, methods)
        CHARACTER(len=*),                            INTENT(IN) :: where
        INTEGER,                                     INTENT(IN) :: num_surface_types
        INTEGER,           DIMENSION(:),             INTENT(IN) :: grid_size
        INTEGER,                           OPTIONAL, INTENT(IN) :: my_bottom_model
        INTEGER(c_int),                    OPTIONAL, INTENT(IN) :: flux
        CHARACTER(len=20), DIMENSION(:,:), OPTIONAL, INTENT(IN) :: methods
        CHARACTER(len=256) :: msg
        INTEGER :: i
        IF (.NOT. c_associated(engine)) CALL contract_error(where, &
            'no flux engine attached (call fcx_attach once all fields are allocated, after flux_calculator.F90:761)')
        IF (num_surface_types /= att_types) THEN
            WRITE (msg, '(A,I0,A,I0)') 'num_surface_types ', num_surface_types, ' but the engine was attached with ', &
                att_types
            CALL contract_error(where, TRIM(msg))
        ENDIF
        IF (SIZE(grid_size) < 3) CALL contract_error(where, 'grid_size has fewer than 3 grids')
        IF (ANY(grid_size(1:3) /= att_grid)) THEN
            WRITE (msg, '(A,3(1X,I0),A,3(1X,I0))') 'grid_size', grid_size(1:3), ' but the engine was attached with', &
                att_grid
            CALL contract_error(where, TRIM(msg))
        ENDIF
        IF (PRESENT(my_bottom_model)) THEN
            IF (my_bottom_model /= att_model) THEN
                WRITE (msg, '(A,I0,A,I0)') 'my_bottom_model ', my_bottom_model, ' but the engine was attached with ', &
                    att_model
                CALL contract_error(where, TRIM(msg))
            ENDIF
        ENDIF
        IF (PRESENT(methods) .AND. PRESENT(flux) .AND. PRESENT(my_bottom_model)) THEN
            DO i = 1, num_surface_types
                IF (TRIM(methods(my_bottom_model, i)) /= TRIM(att_methods(flux, i))) THEN
                    WRITE (msg, '(A,I0,5A)') 'method table differs from the attached one: surface type ', i, &
                        ' is "', TRIM(methods(my_bottom_model, i)), '", attached "', TRIM(att_methods(flux, i)), '"'
                    CALL contract_error(where, TRIM(msg))
                ENDIF
            ENDDO
        ENDIF
    END SUBROUTINE require

    SUBROUTINE set_table(flux, methods, my_bottom_model, num_surface_types)
        INTEGER(c_int),                          INTENT(IN) :: flux
        CHARACTER(len=20), DIMENSION(:,:),       INTENT(IN) :: methods
        INTEGER,                                 INTENT(IN) :: my_bottom_model, num_surface_types
        INTEGER :: i
        INTEGER(c_int) :: m
        DO i = 1, num_surface_types
            m = fcx_method_id(methods(my_bottom_model, i))
            IF (m < 0) CALL stop_run('Method ' // TRIM(methods(my_bottom_model, i)) // ' is not known.')
            CALL check(fcx_set_method(engine, flux, INT(i, c_int), m), 'fcx_set_method')
            att_methods(flux, i) = methods(my_bottom_model, i)
        ENDDO
    END SUBROUTINE set_table

    ! Bind every ASSOCIATED local_field slot (aliases = identical addresses), the method
    ! tables, the bias corrections and the rank-local regridding matrices.
    SUBROUTINE fcx_attach(my_bottom_model, num_surface_types, grid_size, local_field,          &
                          which_spec_vapor_surface_t, which_spec_vapor_surface_u,            &
                          which_spec_vapor_surface_v, which_flux_mass_evap,                  &
                          which_flux_heat_latent, which_flux_heat_sensible,                  &
                          which_flux_momentum, which_flux_radiation_blackbody,               &
                          lcorrection, correction_init_date, corrections_mass_evap,          &
                          regrid_u_to_t_matrix, regrid_v_to_t_matrix,                        &
                          regrid_t_to_u_matrix, regrid_t_to_v_matrix, device)
        INTEGER,                                  INTENT(IN) :: my_bottom_model, num_surface_types
        INTEGER,                 DIMENSION(:),    INTENT(IN) :: grid_size
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(IN), TARGET :: local_field
        CHARACTER(len=20),       DIMENSION(:,:),  INTENT(IN) :: which_spec_vapor_surface_t, &
            which_spec_vapor_surface_u, which_spec_vapor_surface_v, which_flux_mass_evap,    &
            which_flux_heat_latent, which_flux_heat_sensible, which_flux_momentum,           &
            which_flux_radiation_blackbody
        LOGICAL,                                  INTENT(IN) :: lcorrection
        INTEGER,                                  INTENT(IN) :: correction_init_date
        REAL(kind=wp), DIMENSION(:,:), TARGET,    INTENT(IN), OPTIONAL :: corrections_mass_evap ! (12, grid_size(1))
        TYPE(sparse_regridding_matrix),           INTENT(IN), OPTIONAL, TARGET :: regrid_u_to_t_matrix, &
            regrid_v_to_t_matrix, regrid_t_to_u_matrix, regrid_t_to_v_matrix
        INTEGER,                                  INTENT(IN), OPTIONAL :: device
        INTEGER(c_int32_t) :: gs(3)
        INTEGER(c_int) :: dev, flags, mask
        INTEGER :: s, g, v
        REAL(c_double), ALLOCATABLE, TARGET :: corr_d(:,:)

        IF (c_associated(engine)) CALL fcx_detach()
        gs = INT(grid_size(1:3), c_int32_t)
        att_model = my_bottom_model
        att_types = num_surface_types
        att_grid = grid_size(1:3)
        att_methods = ''
        dev = 0
        IF (PRESENT(device)) dev = INT(device, c_int)
        CALL check(fcx_create(dev, INT(num_surface_types, c_int), gs, engine), 'fcx_create')
        ! the NO_USE_DOUBLE_PRECISION build (basic:21-25) keeps REAL(4) fields: fp32 engine
        IF (wp == c_float) CALL check(fcx_set_precision(engine, FCX_PRECISION_F32), 'fcx_set_precision')

        CALL set_table(FCX_SPEC_VAPOR_SURFACE_T, which_spec_vapor_surface_t, my_bottom_model, num_surface_types)
        CALL set_table(FCX_SPEC_VAPOR_SURFACE_U, which_spec_vapor_surface_u, my_bottom_model, num_surface_types)
        CALL set_table(FCX_SPEC_VAPOR_SURFACE_V, which_spec_vapor_surface_v, my_bottom_model, num_surface_types)
        CALL set_table(FCX_FLUX_MASS_EVAP, which_flux_mass_evap, my_bottom_model, num_surface_types)
        CALL set_table(FCX_FLUX_HEAT_LATENT, which_flux_heat_latent, my_bottom_model, num_surface_types)
        CALL set_table(FCX_FLUX_HEAT_SENSIBLE, which_flux_heat_sensible, my_bottom_model, num_surface_types)
        CALL set_table(FCX_FLUX_MOMENTUM, which_flux_momentum, my_bottom_model, num_surface_types)
        CALL set_table(FCX_FLUX_RADIATION_BLACKBODY, which_flux_radiation_blackbody, my_bottom_model, &
                       num_surface_types)

        ! local_field(0:MAX_SURFACE_TYPES, 3)%var(MAX_VARNAMES) (flux_calculator.F90:159)
        DO s = 0, MAX_SURFACE_TYPES
            DO g = 1, 3
                DO v = 1, MAX_VARNAMES
                    IF (.NOT. ASSOCIATED(local_field(s,g)%var(v)%field)) CYCLE
                    IF (SIZE(local_field(s,g)%var(v)%field) == 0) CYCLE
                    flags = FCX_MEM_HOST
                    IF (local_field(s,g)%var(v)%allocated) flags = IOR(flags, FCX_ALLOCATED)
                    CALL check(fcx_bind_field(engine, INT(s, c_int), INT(g, c_int), INT(v, c_int),  &
                                              c_loc(local_field(s,g)%var(v)%field(1)),          &
                                              INT(SIZE(local_field(s,g)%var(v)%field), c_int64_t), &
                                              flags), 'fcx_bind_field')
                    mask = 0
                    IF (local_field(s,g)%var(v)%put_to_t_grid) mask = IOR(mask, 1)
                    IF (local_field(s,g)%var(v)%put_to_u_grid) mask = IOR(mask, 2)
                    IF (local_field(s,g)%var(v)%put_to_v_grid) mask = IOR(mask, 4)
                    IF (mask /= 0) CALL check(fcx_set_put_to(engine, INT(s, c_int), INT(g, c_int), &
                                                             INT(v, c_int), mask), 'fcx_set_put_to')
                ENDDO
            ENDDO
        ENDDO

        ! bias_corrections: corrections(E_MASS_EVAP_CORRECTION, :, :) is (12, grid_size(1))
        IF (lcorrection .AND. PRESENT(corrections_mass_evap)) THEN
            ! the C ABI takes the corrections as double (copied at the call)
            corr_d = REAL(corrections_mass_evap, c_double)
            CALL check(fcx_set_corrections(engine, 1_c_int, INT(correction_init_date, c_int32_t),  &
                                           c_loc(corr_d(1,1)),                                   &
                                           INT(grid_size(1), c_int64_t), FCX_CORR_CELL_MAJOR),    &
                       'fcx_set_corrections')
            DEALLOCATE(corr_d)
        ENDIF

        IF (PRESENT(regrid_u_to_t_matrix)) CALL set_matrix(FCX_U_TO_T, regrid_u_to_t_matrix)
        IF (PRESENT(regrid_v_to_t_matrix)) CALL set_matrix(FCX_V_TO_T, regrid_v_to_t_matrix)
        IF (PRESENT(regrid_t_to_u_matrix)) CALL set_matrix(FCX_T_TO_U, regrid_t_to_u_matrix)
        IF (PRESENT(regrid_t_to_v_matrix)) CALL set_matrix(FCX_T_TO_V, regrid_t_to_v_matrix)
    END SUBROUTINE fcx_attach

    SUBROUTINE set_matrix(which, m)
        INTEGER(c_int),                         INTENT(IN) :: which
        TYPE(sparse_regridding_matrix), TARGET, INTENT(IN) :: m
        ! the C ABI takes double weights (copied at the call); REAL(wp) may be REAL(4)
        REAL(c_double), ALLOCATABLE, TARGET :: w8(:)
        IF (m%num_elements <= 0) RETURN
        ALLOCATE(w8(m%num_elements))
        w8 = REAL(m%weight%field(1:m%num_elements), c_double)
        CALL check(fcx_set_regrid_matrix(engine, which, INT(m%num_elements, c_int64_t),          &
                                         c_loc(m%src_index%field(1)), c_loc(m%dst_index%field(1)), &
                                         c_loc(w8(1))), 'fcx_set_regrid_matrix')
        DEALLOCATE(w8)
    END SUBROUTINE set_matrix

    ! An input field the namelist gave a value instead of a sender (val_bottom_var_* /
    ! val_atmos_var_* > -0.99e20, flux_calculator.F90:444-549: init_localvar fills it once, no
    ! model ever sends it).  Called between fcx_attach and fcx_commit_engine, once per such
    ! field, with the local_field fcx_attach bound: the array must hold `value` in every cell
    ! (checked here, once; a host that changed it has no constant and the run stops), and from
    ! then on the engine neither reads nor writes it -- no upload, no staging, no mapping.
    ! Aliases (distribute_input_field, basic:334-358) follow: every slot bound to the same
    ! address becomes the constant, so an atmosphere constant is declared once, for type 0.
    SUBROUTINE fcx_declare_constant(surface_type, which_grid, my_idx, value, local_field)
        INTEGER,                                  INTENT(IN) :: surface_type, which_grid, my_idx
        REAL(kind=wp),                            INTENT(IN) :: value
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(IN) :: local_field
        CHARACTER(len=160) :: msg
        IF (.NOT. c_associated(engine)) CALL contract_error('fcx_declare_constant', 'no flux engine attached')
        IF (surface_type < 0 .OR. surface_type > MAX_SURFACE_TYPES .OR. which_grid < 1 .OR. which_grid > 3 .OR. &
            my_idx < 1 .OR. my_idx > MAX_VARNAMES) CALL contract_error('fcx_declare_constant', 'slot out of range')
        IF (.NOT. ASSOCIATED(local_field(surface_type, which_grid)%var(my_idx)%field)) &
            CALL contract_error('fcx_declare_constant', 'the field is not associated')
        IF (ANY(local_field(surface_type, which_grid)%var(my_idx)%field /= value)) THEN
            WRITE (msg, '(A,I0,A,I0,A,I0,A,ES23.15)') 'local_field(', surface_type, ',', which_grid, ')%var(', my_idx, &
                ') does not hold the declared constant in every cell: ', value
            CALL contract_error('fcx_declare_constant', TRIM(msg))
        ENDIF
        CALL check(fcx_bind_constant(engine, INT(surface_type, c_int), INT(which_grid, c_int), INT(my_idx, c_int), &
                                     REAL(value, c_double)), 'fcx_bind_constant')
    END SUBROUTINE fcx_declare_constant

    ! A model grid -> exchange grid mapping of received fields (the links of a
    ! mappings/remap_<grid>_<model>_to_exchangegrid.nc file, which the host reads): link k carries
    ! weight(k) * source(src_cell(k)) to exchange cell dst_cell(k) of which_grid, both 1-based and
    ! local to this rank, as the regridding matrices are.  n_src: cells of the model-grid arrays
    ! on this rank.  Called between fcx_attach and fcx_commit_engine; map is what
    ! fcx_declare_received takes.
    SUBROUTINE fcx_define_receive_map(which_grid, n_src, src_cell, dst_cell, weight, map)
        INTEGER,               INTENT(IN)  :: which_grid, n_src
        INTEGER, DIMENSION(:), INTENT(IN)  :: src_cell, dst_cell
        REAL(kind=wp), DIMENSION(:), INTENT(IN) :: weight
        INTEGER,               INTENT(OUT) :: map
        INTEGER(c_int32_t), ALLOCATABLE, TARGET :: s0(:), d0(:)
        REAL(c_double),     ALLOCATABLE, TARGET :: w0(:)
        INTEGER(c_int32_t) :: id
        INTEGER :: n
        IF (.NOT. c_associated(engine)) CALL contract_error('fcx_define_receive_map', 'no flux engine attached')
        n = SIZE(src_cell)
        IF (SIZE(dst_cell) /= n .OR. SIZE(weight) /= n) &
            CALL contract_error('fcx_define_receive_map', 'src_cell, dst_cell and weight differ in length')
        ALLOCATE (s0(MAX(n, 1)), d0(MAX(n, 1)), w0(MAX(n, 1)))
        s0(1:n) = INT(src_cell - 1, c_int32_t)
        d0(1:n) = INT(dst_cell - 1, c_int32_t)
        w0(1:n) = REAL(weight, c_double)
        CALL check(fcx_add_receive_map(engine, INT(which_grid, c_int), INT(n_src, c_int64_t), INT(n, c_int64_t), &
                                       C_LOC(s0), C_LOC(d0), C_LOC(w0), id), 'fcx_add_receive_map')
        map = INT(id)
    END SUBROUTINE fcx_define_receive_map

    ! An input field the host receives on its MODEL's grid: the host's oasis_get of the field
    ! writes `source` (n_src cells of the map) instead of local_field's exchange-grid array, with
    ! no OASIS remapping on the way, and the engine applies the map on the device at the start
    ! of `phase` (FCX_PHASE_EARLY where input_field%early, else FCX_PHASE_NORMAL).  Called between
    ! fcx_attach and fcx_commit_engine with the local_field fcx_attach bound.  From then on the
    ! engine neither reads nor writes the exchange-grid array; aliases (distribute_input_field,
    ! basic:334-358) follow, so an atmosphere field is declared once, for surface type 0.
    ! `source` must stay allocated until fcx_detach (fcx_allocate_field memory, or the heap).
    SUBROUTINE fcx_declare_received(surface_type, which_grid, my_idx, map, phase, source, local_field)
        INTEGER,                                  INTENT(IN) :: surface_type, which_grid, my_idx, map
        INTEGER(c_int),                           INTENT(IN) :: phase
        REAL(kind=wp), DIMENSION(:), POINTER,     INTENT(IN) :: source
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(IN) :: local_field
        IF (.NOT. c_associated(engine)) CALL contract_error('fcx_declare_received', 'no flux engine attached')
        IF (surface_type < 0 .OR. surface_type > MAX_SURFACE_TYPES .OR. which_grid < 1 .OR. which_grid > 3 .OR. &
            my_idx < 1 .OR. my_idx > MAX_VARNAMES) CALL contract_error('fcx_declare_received', 'slot out of range')
        IF (.NOT. ASSOCIATED(local_field(surface_type, which_grid)%var(my_idx)%field)) &
            CALL contract_error('fcx_declare_received', 'the field is not associated')
        IF (.NOT. ASSOCIATED(source)) CALL contract_error('fcx_declare_received', 'the source array is not associated')
        IF (SIZE(source) < 1) CALL contract_error('fcx_declare_received', 'the source array is empty')
        CALL check(fcx_bind_received(engine, INT(map, c_int32_t), phase, INT(surface_type, c_int), &
                                     INT(which_grid, c_int), INT(my_idx, c_int), C_LOC(source(1)), &
                                     INT(SIZE(source), c_int64_t), FCX_MEM_HOST), 'fcx_bind_received')
    END SUBROUTINE fcx_declare_received

    ! The outputs the host never sends.  output_field holds what the send_to_* / name_send_*
    ! tables select (add_output_field, basic:170-284); every other computed flux of surface types
    ! 1..T -- QSUR is one in every set-up -- is calculated, downloaded and left unread.  Called
    ! between fcx_attach and fcx_commit_engine, where fcx_declare_constant is called, with the
    ! host's own output_field and the local_field fcx_attach bound: each computed array that no
    ! output_field entry points to (compared by address, so uniform and 'copy' aliases count as
    ! sent) and that is not a regridding source is declared FCX_OUT_UNREAD.  From the commit on
    ! the engine neither writes nor reads those arrays: the fluxes stay on the device, and where
    ! nothing but the launch's own registers consumes one it is not stored at all (fcx.h,
    ! fcx_set_output_use).  A host that reads such an array itself must not call this.
    SUBROUTINE fcx_select_outputs(num_output_fields, output_field, local_field)
        INTEGER,                                  INTENT(IN) :: num_output_fields
        TYPE(io_fields_type),    DIMENSION(:),    INTENT(IN) :: output_field
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(IN), TARGET :: local_field
        INTEGER :: computed(7), s, g, k, v, j
        LOGICAL :: sent
        TYPE(c_ptr) :: addr
        IF (.NOT. c_associated(engine)) CALL contract_error('fcx_select_outputs', 'no flux engine attached')
        computed = [idx_QSUR, idx_MEVA, idx_HLAT, idx_HSEN, idx_RBBR, idx_UMOM, idx_VMOM]
        DO s = 1, att_types
            DO g = 1, 3
                DO k = 1, SIZE(computed)
                    v = computed(k)
                    IF (v < 1 .OR. v > MAX_VARNAMES) CYCLE
                    IF (.NOT. ASSOCIATED(local_field(s,g)%var(v)%field)) CYCLE
                    IF (SIZE(local_field(s,g)%var(v)%field) == 0) CYCLE
                    IF (local_field(s,g)%var(v)%put_to_t_grid .OR. local_field(s,g)%var(v)%put_to_u_grid .OR. &
                        local_field(s,g)%var(v)%put_to_v_grid) CYCLE
                    addr = c_loc(local_field(s,g)%var(v)%field(1))
                    sent = .FALSE.
                    DO j = 1, MIN(num_output_fields, SIZE(output_field))
                        IF (.NOT. ASSOCIATED(output_field(j)%field)) CYCLE
                        IF (SIZE(output_field(j)%field) == 0) CYCLE
                        IF (c_associated(addr, c_loc(output_field(j)%field(1)))) sent = .TRUE.
                    ENDDO
                    IF (sent) CYCLE
                    CALL check(fcx_set_output_use(engine, INT(s, c_int), INT(g, c_int), INT(v, c_int), FCX_OUT_UNREAD), &
                               'fcx_set_output_use')
                ENDDO
            ENDDO
        ENDDO
    END SUBROUTINE fcx_select_outputs

    ! output_field(j) with surface_type 0 (flux_calculator.F90:909-918, 999-1008)
    SUBROUTINE fcx_register_average(early, which_grid, my_idx)
        LOGICAL, INTENT(IN) :: early
        INTEGER, INTENT(IN) :: which_grid, my_idx
        INTEGER(c_int) :: phase
        phase = FCX_PHASE_NORMAL
        IF (early) phase = FCX_PHASE_EARLY
        CALL check(fcx_add_average(engine, phase, INT(which_grid, c_int), INT(my_idx, c_int)), &
                   'fcx_add_average')
    END SUBROUTINE fcx_register_average

    ! The non-finite guard (FCX_OPT_CHECK_FINITE), before fcx_commit_engine.  what: 1 the outputs
    ! of every phase, 3 its inputs too, 0 off.  A phase that finds a NaN or an Inf then fails
    ! like any other engine error: fcx_run_phase / fcx_finish_phase hand the message -- phase,
    ! field, cell, value and counts, e.g. "phase 2: TATM(1,t) cell 4097 = nan (1 NaN, 0 Inf of
    ! 8200 cells)" -- to the registered abort routine (fcx_register_abort) before the ERROR STOP.
    SUBROUTINE fcx_check_finite(what)
        INTEGER, INTENT(IN) :: what
        CALL check(fcx_set_option(engine, FCX_OPT_CHECK_FINITE, INT(what, c_int64_t)), 'fcx_check_finite')
    END SUBROUTINE fcx_check_finite

    ! Atmosphere sums that do not depend on the number of ranks (FCX_OPT_ATMOS_INVARIANT), before
    ! fcx_commit_engine.  max_terms: the largest number of exchange cells of any atmosphere cell
    ! shared between ranks, the same on every rank (an MPI_Allreduce(MAX) of the ranks' own
    ! counts); left_pos: how many exchange cells of this rank's first atmosphere cell lie on lower
    ! ranks (a prefix over the ranks holding that cell; 0 when the cell begins here).
    ! INTEGRATION.md section 3 shows both.  The boundary slots the host hands over with
    ! fcx_set_atmos_shared then need fcx_atmos_columns doubles per boundary.
    SUBROUTINE fcx_define_atmos_terms(max_terms, left_pos)
        INTEGER, INTENT(IN) :: max_terms, left_pos
        IF (.NOT. c_associated(engine)) CALL contract_error('fcx_define_atmos_terms', 'no flux engine attached')
        CALL check(fcx_set_option(engine, FCX_OPT_ATMOS_INVARIANT, 1_c_int64_t), 'fcx_define_atmos_terms')
        CALL check(fcx_set_atmos_terms(engine, INT(max_terms, c_int32_t), INT(left_pos, c_int32_t)), &
                   'fcx_set_atmos_terms')
    END SUBROUTINE fcx_define_atmos_terms

    ! The attached engine, for what the module has no routine of its own for: a host that adds the
    ! exchange -> atmosphere accumulation calls fcx_set_atmos_map, fcx_add_atmos_field,
    ! fcx_set_atmos_shared and fcx_atmos_finish of fcx_c_api on it (INTEGRATION.md section 5).
    ! c_null_ptr when no engine is attached.
    FUNCTION fcx_engine_handle() RESULT(h)
        TYPE(c_ptr) :: h
        h = engine
    END FUNCTION fcx_engine_handle

    ! MINVAL / MAXVAL of local_field(surface_type, which_grid)%var(my_idx) as the engine holds
    ! it on the device, for a host's own DEBUG lines (flux_calculator.F90:879-881, 921-924,
    ! 949-951, 1011-1013): the received field the calculation saw, a constant, an output that
    ! never crosses the host link.  n_bad: cells holding a NaN or an Inf (they take no part in
    ! vmin / vmax, which are NaN when no cell holds a number).
    SUBROUTINE fcx_field_range_of(surface_type, which_grid, my_idx, vmin, vmax, n_bad)
        INTEGER,  INTENT(IN)  :: surface_type, which_grid, my_idx
        REAL(wp), INTENT(OUT) :: vmin, vmax
        INTEGER,  INTENT(OUT) :: n_bad
        INTEGER(c_int32_t) :: slot(3)
        TYPE(fcx_field_range) :: r(1)
        slot = [INT(surface_type, c_int32_t), INT(which_grid, c_int32_t), INT(my_idx, c_int32_t)]
        CALL check(fcx_field_ranges(engine, 1_c_int32_t, slot, r), 'fcx_field_ranges')
        vmin = REAL(r(1)%vmin, wp)
        vmax = REAL(r(1)%vmax, wp)
        n_bad = INT(r(1)%n_nan + r(1)%n_inf)
    END SUBROUTINE fcx_field_range_of

    ! The cell areas of exchange grid which_grid for the flux budgets: grid_area as the host holds
    ! it for oasis_write_area (flux_calculator.F90:791-793), this rank's window of it, at least
    ! grid_size(which_grid) values.  Before or after fcx_commit_engine; again to replace them.
    SUBROUTINE fcx_declare_areas(which_grid, area)
        INTEGER,                INTENT(IN) :: which_grid
        REAL(wp), DIMENSION(:), INTENT(IN) :: area
        REAL(c_double), ALLOCATABLE :: a(:)
        a = REAL(area, c_double)
        CALL check(fcx_set_areas(engine, INT(which_grid, c_int), a, SIZE(a, KIND=c_int64_t)), 'fcx_set_areas')
    END SUBROUTINE fcx_declare_areas

    ! The integral of local_field(surface_type, which_grid)%var(my_idx) over the grid as the engine
    ! holds it on the device: sum_j area(j) * field(j) (weighted) or sum_j field(j), exact and
    ! rounded once -- the same bits whatever the decomposition.  value is this rank's; hosts that
    ! want the global budget add the ranks' fcx_exact_sum with MPI_SUM (fcx_field_integrals,
    ! fcx_sum_merge, fcx_sum_value of fcx_c_api).  Terms that are NaN or +-Inf are left out of the
    ! sum and make value NaN or +-Inf, as fcx_sum_value defines it.
    SUBROUTINE fcx_field_integral_of(surface_type, which_grid, my_idx, weighted, value)
        INTEGER,  INTENT(IN)  :: surface_type, which_grid, my_idx
        LOGICAL,  INTENT(IN)  :: weighted
        REAL(wp), INTENT(OUT) :: value
        INTEGER(c_int32_t) :: slot(3)
        TYPE(fcx_exact_sum) :: s(1)
        REAL(c_double) :: v
        slot = [INT(surface_type, c_int32_t), INT(which_grid, c_int32_t), INT(my_idx, c_int32_t)]
        CALL check(fcx_field_integrals(engine, 1_c_int32_t, slot, MERGE(1_c_int, 0_c_int, weighted), s), &
                   'fcx_field_integrals')
        CALL check(fcx_sum_value(s(1), v), 'fcx_sum_value')
        value = REAL(v, wp)
    END SUBROUTINE fcx_field_integral_of

    ! every plan the engine can launch audited on the host first (fcx_plan_check: a method
    ! that would read an input the set-up left unbound stops here with a named error, before
    ! any device memory is taken), then validation and the device mirrors
    SUBROUTINE fcx_commit_engine()
        CALL check(fcx_plan_check(engine), 'fcx_plan_check')
        CALL check(fcx_commit(engine), 'fcx_commit')
    END SUBROUTINE fcx_commit_engine

    ! One fused phase: upload the phase's inputs, all its fluxes + regrids + type-0
    ! averages in one pass, download its outputs.  phase: FCX_PHASE_EARLY (replaces
    ! flux_calculator.F90:902-918) or FCX_PHASE_NORMAL (replaces :972-1008).
    SUBROUTINE fcx_run_phase(phase)
        INTEGER(c_int), INTENT(IN) :: phase
        CALL check(fcx_step(engine, phase, INT(current_step_time, c_int32_t)), 'fcx_step')
    END SUBROUTINE fcx_run_phase

    ! fcx_run_phase in two halves (fcx_step_async + fcx_synchronize): after fcx_start_phase
    ! the phase's input fields may be overwritten (their values are in the engine); its
    ! output fields hold the results after fcx_finish_phase
    SUBROUTINE fcx_start_phase(phase)
        INTEGER(c_int), INTENT(IN) :: phase
        CALL check(fcx_step_async(engine, phase, INT(current_step_time, c_int32_t)), 'fcx_step_async')
    END SUBROUTINE fcx_start_phase

    ! one input field right after its oasis_get (flux_calculator.F90:876-880, 946-950): the
    ! engine's upload thread stages it while the host receives the next field; the phase that
    ! follows moves only the inputs not handed over.  The array may be overwritten once the
    ! next engine call returns.
    SUBROUTINE fcx_hand_over_field(surface_type, which_grid, my_idx)
        INTEGER, INTENT(IN) :: surface_type, which_grid, my_idx
        CALL check(fcx_upload_field(engine, INT(surface_type, c_int), INT(which_grid, c_int), INT(my_idx, c_int)), &
                   'fcx_upload_field')
    END SUBROUTINE fcx_hand_over_field

    SUBROUTINE fcx_finish_phase()
        CALL check(fcx_synchronize(engine), 'fcx_synchronize')
    END SUBROUTINE fcx_finish_phase

    SUBROUTINE fcx_detach()
        INTEGER(c_int) :: r
        IF (.NOT. c_associated(engine)) RETURN
        r = fcx_destroy(engine)
        engine = c_null_ptr
        att_model = -1
        att_types = -1
        att_grid = -1
    END SUBROUTINE fcx_detach

    !!!!!!!!!! the reference subroutines (flux_calculator_calculate.F90:25-385) !!!!!!!!!!

    SUBROUTINE calc_spec_vapor_surface(my_bottom_model, num_surface_types, which_grid, methods, grid_size, local_field)
        INTEGER,                                  INTENT(IN)    :: my_bottom_model
        INTEGER,                                  INTENT(IN)    :: num_surface_types
        INTEGER,                                  INTENT(IN)    :: which_grid
        CHARACTER(len=20),       DIMENSION(:,:),  INTENT(IN)    :: methods
        INTEGER,                 DIMENSION(:),    INTENT(IN)    :: grid_size
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(INOUT) :: local_field
        IF (which_grid < 1 .OR. which_grid > 3) CALL contract_error('calc_spec_vapor_surface', 'which_grid outside 1..3')
        CALL require('calc_spec_vapor_surface', num_surface_types, grid_size, my_bottom_model, &
                     FCX_SPEC_VAPOR_SURFACE_T + INT(which_grid - 1, c_int), methods)
        CALL check(fcx_calc_spec_vapor_surface(engine, INT(which_grid, c_int)), 'calc_spec_vapor_surface')
    END SUBROUTINE calc_spec_vapor_surface

    SUBROUTINE calc_flux_mass_evap(my_bottom_model, num_surface_types, methods, grid_size, local_field)
        INTEGER,                                  INTENT(IN)    :: my_bottom_model
        INTEGER,                                  INTENT(IN)    :: num_surface_types
        CHARACTER(len=20),       DIMENSION(:,:),  INTENT(IN)    :: methods
        INTEGER,                 DIMENSION(:),    INTENT(IN)    :: grid_size
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(INOUT) :: local_field
        ! the month of the bias correction comes from current_step_time (basic:125)
        CALL require('calc_flux_mass_evap', num_surface_types, grid_size, my_bottom_model, FCX_FLUX_MASS_EVAP, methods)
        CALL check(fcx_calc_flux_mass_evap(engine, INT(current_step_time, c_int32_t)), 'calc_flux_mass_evap')
    END SUBROUTINE calc_flux_mass_evap

    SUBROUTINE calc_flux_heat_latent(my_bottom_model, num_surface_types, methods, grid_size, local_field)
        INTEGER,                                  INTENT(IN)    :: my_bottom_model
        INTEGER,                                  INTENT(IN)    :: num_surface_types
        CHARACTER(len=20),       DIMENSION(:,:),  INTENT(IN)    :: methods
        INTEGER,                 DIMENSION(:),    INTENT(IN)    :: grid_size
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(INOUT) :: local_field
        CALL require('calc_flux_heat_latent', num_surface_types, grid_size, my_bottom_model, FCX_FLUX_HEAT_LATENT, &
                     methods)
        CALL check(fcx_calc_flux_heat_latent(engine), 'calc_flux_heat_latent')
    END SUBROUTINE calc_flux_heat_latent

    SUBROUTINE calc_flux_heat_sensible(my_bottom_model, num_surface_types, methods, grid_size, local_field)
        INTEGER,                                  INTENT(IN)    :: my_bottom_model
        INTEGER,                                  INTENT(IN)    :: num_surface_types
        CHARACTER(len=20),       DIMENSION(:,:),  INTENT(IN)    :: methods
        INTEGER,                 DIMENSION(:),    INTENT(IN)    :: grid_size
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(INOUT) :: local_field
        CALL require('calc_flux_heat_sensible', num_surface_types, grid_size, my_bottom_model, &
                     FCX_FLUX_HEAT_SENSIBLE, methods)
        CALL check(fcx_calc_flux_heat_sensible(engine), 'calc_flux_heat_sensible')
    END SUBROUTINE calc_flux_heat_sensible

    SUBROUTINE calc_flux_momentum_east(my_bottom_model, num_surface_types, which_grid, methods, grid_size, local_field)
        INTEGER,                                  INTENT(IN)    :: my_bottom_model
        INTEGER,                                  INTENT(IN)    :: num_surface_types
        INTEGER,                                  INTENT(IN)    :: which_grid
        CHARACTER(len=20),       DIMENSION(:,:),  INTENT(IN)    :: methods
        INTEGER,                 DIMENSION(:),    INTENT(IN)    :: grid_size
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(INOUT) :: local_field
        CALL require('calc_flux_momentum_east', num_surface_types, grid_size, my_bottom_model, FCX_FLUX_MOMENTUM, &
                     methods)
        CALL check(fcx_calc_flux_momentum_east(engine, INT(which_grid, c_int)), 'calc_flux_momentum_east')
    END SUBROUTINE calc_flux_momentum_east

    SUBROUTINE calc_flux_momentum_north(my_bottom_model, num_surface_types, which_grid, methods, grid_size, local_field)
        INTEGER,                                  INTENT(IN)    :: my_bottom_model
        INTEGER,                                  INTENT(IN)    :: num_surface_types
        INTEGER,                                  INTENT(IN)    :: which_grid
        CHARACTER(len=20),       DIMENSION(:,:),  INTENT(IN)    :: methods
        INTEGER,                 DIMENSION(:),    INTENT(IN)    :: grid_size
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(INOUT) :: local_field
        CALL require('calc_flux_momentum_north', num_surface_types, grid_size, my_bottom_model, FCX_FLUX_MOMENTUM, &
                     methods)
        CALL check(fcx_calc_flux_momentum_north(engine, INT(which_grid, c_int)), 'calc_flux_momentum_north')
    END SUBROUTINE calc_flux_momentum_north

    SUBROUTINE calc_flux_radiation_blackbody(my_bottom_model, num_surface_types, methods, grid_size, local_field)
        INTEGER,                                  INTENT(IN)    :: my_bottom_model
        INTEGER,                                  INTENT(IN)    :: num_surface_types
        CHARACTER(len=20),       DIMENSION(:,:),  INTENT(IN)    :: methods
        INTEGER,                 DIMENSION(:),    INTENT(IN)    :: grid_size
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(INOUT) :: local_field
        CALL require('calc_flux_radiation_blackbody', num_surface_types, grid_size, my_bottom_model, &
                     FCX_FLUX_RADIATION_BLACKBODY, methods)
        CALL check(fcx_calc_flux_radiation_blackbody(engine), 'calc_flux_radiation_blackbody')
    END SUBROUTINE calc_flux_radiation_blackbody

    SUBROUTINE distribute_shortwave_radiation_flux(my_bottom_model, num_surface_types, grid_size, local_field)
        INTEGER,                                  INTENT(IN)    :: my_bottom_model
        INTEGER,                                  INTENT(IN)    :: num_surface_types
        INTEGER,                 DIMENSION(:),    INTENT(IN)    :: grid_size
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(INOUT) :: local_field
        CALL require('distribute_shortwave_radiation_flux', num_surface_types, grid_size, my_bottom_model)
        CALL check(fcx_distribute_shortwave_radiation_flux(engine), 'distribute_shortwave_radiation_flux')
    END SUBROUTINE distribute_shortwave_radiation_flux

    SUBROUTINE average_across_surface_types(which_grid, my_idx, num_surface_types, grid_size, local_field)
        INTEGER,                                  INTENT(IN)    :: which_grid
        INTEGER,                                  INTENT(IN)    :: my_idx
        INTEGER,                                  INTENT(IN)    :: num_surface_types
        INTEGER,                 DIMENSION(:),    INTENT(IN)    :: grid_size
        TYPE(local_fields_type), DIMENSION(0:,:), INTENT(INOUT) :: local_field
        CALL require('average_across_surface_types', num_surface_types, grid_size)
        CALL check(fcx_average_across_surface_types(engine, INT(which_grid, c_int), INT(my_idx, c_int)), &
                   'average_across_surface_types')
    END SUBROUTINE average_across_surface_types

END MODULE flux_calculator_calculate
