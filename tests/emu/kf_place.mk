# TEST INFRASTRUCTURE ONLY: libmpcqp_emu_kf_place.so = the objects of libmpcqp_emu_mheloop.so (mheloop.mk) + the pole placement
# of the Luenberger observer (emu_kf_place.cpp).  A makefile of its own: the other libraries stay WITHOUT that launcher.
include Makefile
libmpcqp_emu_kf_place.so: $(STOCK_OBJS) $(EST_OBJS) emu_explicit.o emu_sim.o emu_est_init.o emu_kf_place.o
-include emu_explicit.d emu_sim.d emu_est_init.d emu_kf_place.d
