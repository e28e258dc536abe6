# build.mk — the rules behind build.sh, which runs make in this directory with OBJ, OUT, HIPCC and FLAGS set.
# One object per translation unit.  The compiler writes each object's depfile (-MMD: the unit's source and every project header it
# read, as paths relative to this directory, so they stay valid when the tree is copied), and those depfiles decide what is stale:
# no list of headers is kept by hand.
UNITS := kernels_cons kernels_cons_wide kernels_cons_linear kernels_cons_linear_wide kernels_append kernels_eig kernels_strip kernels_cov kernels_cov_sparse kernels_sparse kernels_sweep kernels_dense16 \
         kernels_filter kernels_convert kernels_gram kernels_cd kernels_cd_lasso kernels_cd_pin kernels_cd_block kernels_cd_block_group \
         kernels_cd_panel kernels_multi kernels_multi_sparse kernels_glm kernels_cox kernels_factor kernels_relu kernels_relu_sparse kernels_phased \
         kernels_css kernels_bvls kernels_pinball kernels_pinball_sparse kernels_qp_full kernels_bcd design solver test_entries
OBJS := $(UNITS:%=$(OBJ)/%.o)
DEPS := $(OBJS:.o=.d)

$(OUT): $(OBJS)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(OBJS)

# An object is rebuilt when it is missing, when its depfile is missing (the empty rule below then counts as having remade it), and
# when a file the depfile names is newer than the object or gone (-MP gives every header a target, so a deleted one is no error).
# The depfile is written after the object, hence the touch; a failed or interrupted compile leaves no object behind.
$(OBJ)/%.o: %.hip $(OBJ)/%.d
	timeout 600 $(HIPCC) $(FLAGS) -MMD -MP -MF $(OBJ)/$*.d -c $< -o $@ && touch $@
# kernels_bcd packs the float32 values of neighbouring problems side by side, which invites packed float32 instructions; their
# results must be those of the scalar ones bit for bit, so the unit is compiled without them.
$(OBJ)/kernels_bcd.o: FLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops
# kernels_cons_wide computes in double precision and converts float32 values on load only: it has no use for packed float32
# instructions either, and is compiled without them like kernels_bcd.
$(OBJ)/kernels_cons_wide.o: FLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops
$(OBJ)/kernels_cons_linear.o: FLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops
$(OBJ)/kernels_cons_linear_wide.o: FLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops
# kernels_multi_sparse keeps up to eight float32 accumulators side by side per lane: compiled without packed float32 instructions too.
$(OBJ)/kernels_multi_sparse.o: FLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops
$(DEPS): ;
.DELETE_ON_ERROR:
-include $(DEPS)
