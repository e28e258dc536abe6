# build.mk — the rules behind build.sh, which runs make in this directory with OBJ, OUT, HIPCC and FLAGS set.
# One object per translation unit.  The compiler writes each object's depfile (-MMD: the unit's source and every project header it
# read, as paths relative to this directory, so they stay valid when the tree is copied), and those depfiles decide what is stale:
# no list of headers is kept by hand.
UNITS := kernels_cons kernels_append kernels_eig kernels_strip kernels_cov kernels_cov_sparse kernels_sparse kernels_sweep \
         kernels_filter kernels_convert kernels_gram kernels_cd kernels_cd_lasso kernels_cd_pin kernels_cd_block kernels_cd_block_group \
         kernels_cd_panel kernels_multi kernels_glm kernels_cox kernels_factor kernels_relu kernels_relu_sparse kernels_phased \
         kernels_css kernels_bvls kernels_pinball kernels_pinball_sparse kernels_qp_full design solver test_entries
OBJS := $(UNITS:%=$(OBJ)/%.o)
DEPS := $(OBJS:.o=.d)

$(OUT): $(OBJS)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(OBJS)

# An object is rebuilt when it is missing, when its depfile is missing (the empty rule below then counts as having remade it), and
# when a file the depfile names is newer than the object or gone (-MP gives every header a target, so a deleted one is no error).
# The depfile is written after the object, hence the touch; a failed or interrupted compile leaves no object behind.
$(OBJ)/%.o: %.hip $(OBJ)/%.d
	timeout 600 $(HIPCC) $(FLAGS) -MMD -MP -MF $(OBJ)/$*.d -c $< -o $@ && touch $@
$(DEPS): ;
.DELETE_ON_ERROR:
-include $(DEPS)
