# TEST INFRASTRUCTURE ONLY: libmpcqp_emu_mheloop.so = the objects of libmpcqp_emu_sim.so (sim.mk) + the estimator half of
# initstate! (emu_est_init.cpp).  A makefile of its own: the other libraries stay WITHOUT that launcher.
include Makefile
libmpcqp_emu_mheloop.so: $(STOCK_OBJS) $(EST_OBJS) emu_explicit.o emu_sim.o emu_est_init.o
-include emu_explicit.d emu_sim.d emu_est_init.d
